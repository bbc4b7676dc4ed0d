from .runs import DeviceRunOps, HostRunOps, RunMap, host_runs_encode  # noqa: F401
