from .uni_pc import unipc_plan  # noqa: F401
from .sampler import UniPC, UniPCSampler  # noqa: F401
