from .dpm_solver import NoiseScheduleVP, solver_plan  # noqa: F401
from .sampler import DPMSolverSampler  # noqa: F401
from .solver import DPM_Solver, model_wrapper  # noqa: F401
