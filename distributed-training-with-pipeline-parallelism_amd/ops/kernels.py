"""Op wrappers: GPU -> HIP kernels in ``_C.so``; CPU -> PyTorch f32 reference math.

A facade with no logic: the ops live in one module per kernel family, named after their
bindings in csrc/bindings/ (``_base`` holds the loader and what the families share).  This
module re-exports every public name, and the private ones that tools and tests reach.

The names here are copies made at import.  Rebinding one on this module does not reach the
family that owns it: stand in for the extension at ``_base._EXT``, flip a switch
(``GEMM_BACKEND``, ``GEMM_V``, ``_WGRAD_GROUP``, ``_WGRAD_GROUP3``, ``_GROUP3_MIN_T``) in the
module that defines it."""
from . import _base, attention, elementwise_optim, gemm, gemm_f32, generate, norm_loss_embed, quant, wgrad
from ._base import *  # noqa: F401,F403
from ._base import _ext, _gpu  # noqa: F401
from .attention import *  # noqa: F401,F403
from .attention import _cpu_attn_drop  # noqa: F401
from .elementwise_optim import *  # noqa: F401,F403
from .gemm import *  # noqa: F401,F403
from .gemm import _gemm  # noqa: F401
from .gemm_f32 import *  # noqa: F401,F403
from .gemm_f32 import _gemm_f32, _mha_projected  # noqa: F401
from .generate import *  # noqa: F401,F403
from .norm_loss_embed import *  # noqa: F401,F403
from .quant import *  # noqa: F401,F403
from .wgrad import *  # noqa: F401,F403

__all__ = [n for m in (_base, norm_loss_embed, gemm, gemm_f32, wgrad, quant, elementwise_optim, attention, generate)
           for n in m.__all__]
