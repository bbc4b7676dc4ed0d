from .outlines import DeviceOutlineOps, HostOutlineOps, Outline, host_outline  # noqa: F401
from .polygons import Polygons, host_simplify  # noqa: F401
from .runs import DeviceRunOps, HostRunOps, RunMap, host_runs_decode, host_runs_encode, stack_objects  # noqa: F401
