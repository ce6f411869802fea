"""Weight-gradient jobs kept as data and the planner that groups them into the grouped dW
launches (csrc/bindings/gemm.cpp ``gemm_tt_grouped`` / ``gemm_dw_grouped``).

The switches ``_WGRAD_GROUP``, ``_WGRAD_GROUP3`` and ``_GROUP3_MIN_T`` live here.  What this
module takes from others -- ``_base._gpu``, ``gemm.GEMM_BACKEND``, ``gemm.linear_dw``,
``elementwise_optim.colsum`` -- it looks up in the owning module when it runs, so a test that
rebinds one of them there is seen here."""
from __future__ import annotations

import os

import torch

from . import _base, elementwise_optim, gemm
from ._base import _ext

__all__ = ["DW", "ColSum", "plan_wjobs", "run_wjobs"]

# MIPIPE_WGRAD_GROUP=0: every weight-gradient GEMM of a job list in its own launch
_WGRAD_GROUP = os.environ.get("MIPIPE_WGRAD_GROUP", "1") != "0"
# MIPIPE_WGRAD_GROUP3=0: the long-token weight-gradient GEMMs of a job list one launch (and
# one split-K reduce) each, as before the grouped 256x256 engine
_WGRAD_GROUP3 = os.environ.get("MIPIPE_WGRAD_GROUP3", "1") != "0"
_GROUP_MAX = 8
# token count from which a job list's dW GEMMs share one grouped 256x256 launch: the
# microbatch of a PP > 1 rank (16K tokens), where the per-GEMM planner is down to 9-36
# K-tiles per workgroup; below it the per-GEMM split-K plan stays
_GROUP3_MIN_T = 16384


class DW:
    """A weight-gradient job ``dw (f32) += alpha * dy^T x`` kept as data, so that
    :func:`run_wjobs` can issue the short-token ones of a job list as ONE grouped launch
    (csrc/include/mp_gemm_small.h ``gemms_tt_grouped_kernel``) and the long-token ones as one
    grouped 256x256 split-K launch (``gemm3_tt_grouped_kernel``).  Calling it runs it alone."""
    __slots__ = ("dy", "x", "dw", "alpha")

    def __init__(self, dy: torch.Tensor, x: torch.Tensor, dw: torch.Tensor, alpha: float = 1.0):
        self.dy, self.x, self.dw, self.alpha = dy, x, dw, alpha

    def __call__(self):
        gemm.linear_dw(self.dy, self.x, self.dw, self.alpha)

    def _tt_operands(self) -> bool:
        dy, x, dw = self.dy, self.x, self.dw
        if not (_base._gpu(dy) and dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and dw.dtype == torch.float32):
            return False
        if dy.dim() != 2 or x.dim() != 2 or dw.dim() != 2:
            return False
        if dy.stride(1) != 1 or x.stride(1) != 1 or dw.stride(1) != 1:
            return False
        T, N = dy.shape
        return not (T % 64 or N % 8 or x.shape[1] % 8)

    def tiles256(self) -> int:
        return ((self.dy.shape[1] + 255) // 256) * ((self.x.shape[1] + 255) // 256)

    def groupable(self) -> bool:
        """Short reductions (<= 4096 tokens) over few 256x256 output tiles: the shapes the
        planner sends to the small 64x64 TT engine (mp_gemm_plan.h plan_tt, cfg 13)."""
        return self._tt_operands() and self.dy.shape[0] <= 4096 and self.tiles256() < 64

    def groupable3(self) -> bool:
        """Long reductions (>= ``_GROUP3_MIN_T`` tokens) onto fewer 256x256 tiles than the
        chip has CUs: alone such a GEMM needs a deep split-K to cover the chip, together with
        its layer's other dW GEMMs a shallow one (an output of >= 256 tiles, the LM head's,
        fills the chip by itself and keeps its own launch)."""
        return self._tt_operands() and self.dy.shape[0] >= _GROUP3_MIN_T and self.tiles256() < 256


class ColSum:
    """A bias-gradient job ``dbias (f32) += column sums of x`` kept as data like :class:`DW`:
    :func:`plan_wjobs` can see which dW job reads the same ``dy``.  Calling it runs it."""
    __slots__ = ("x", "dbias")

    def __init__(self, x: torch.Tensor, dbias: torch.Tensor):
        self.x, self.dbias = x, dbias

    def __call__(self):
        elementwise_optim.colsum(self.x, self.dbias)


def plan_wjobs(jobs):
    """Split a job list into ``(small, long, rest)``: ``small`` -- lists of <= 8 short-token
    DW jobs of one alpha for the 64x64 grouped engine; ``long`` -- lists of 2..8 long-token
    DW jobs of one (alpha, T) for the grouped 256x256 split-K engine, in list order, so a
    deferred list that spans layers is cut into per-T chunks of the group size; ``rest`` --
    everything else (single DW jobs, bias sums, callables) in list order."""
    small, long_ = [], []
    if not (_WGRAD_GROUP and gemm.GEMM_BACKEND != "blas"):
        return small, long_, list(jobs)
    sg, lg = {}, {}
    for j in jobs:
        if _WGRAD_GROUP3 and isinstance(j, DW) and j.groupable3():
            lg.setdefault((j.alpha, j.dy.shape[0]), []).append(j)
        elif isinstance(j, DW) and j.groupable():
            sg.setdefault(j.alpha, []).append(j)
    for g in sg.values():
        if len(g) > 1:
            small.extend(g[i:i + _GROUP_MAX] for i in range(0, len(g), _GROUP_MAX))
    for g in lg.values():
        parts = [g[i:i + _GROUP_MAX] for i in range(0, len(g), _GROUP_MAX)]
        long_.extend(part for part in parts if len(part) > 1)
    grouped = {id(j) for part in small + long_ for j in part}
    return small, long_, [j for j in jobs if id(j) not in grouped]


def _run_group_small(part) -> None:
    _ext().gemm_tt_grouped([j.dy for j in part], [j.x for j in part], [j.dw for j in part], float(part[0].alpha))


def _run_group_long(part) -> None:
    _ext().gemm_dw_grouped([j.dy for j in part], [j.x for j in part], [j.dw for j in part], float(part[0].alpha))


def run_wjobs(jobs) -> None:
    """Run a list of weight-gradient jobs (:class:`DW` and :class:`ColSum` objects and plain
    callables).  The groupable DW jobs go out as grouped launches of up to 8 GEMMs
    (:func:`plan_wjobs`); everything else runs in list order.  Jobs of one list write
    distinct gradient buffers, so the reordering is exact."""
    if not jobs:
        return
    small, long_, rest = plan_wjobs(jobs)
    for part in small:
        _run_group_small(part)
    for part in long_:
        _run_group_long(part)
    for j in rest:
        j()
