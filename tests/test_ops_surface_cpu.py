"""The public surface of ``mipipe.ops`` and of its facade ``ops.kernels``: the set of names, for
every function and class ``str(inspect.signature(...))`` and the first line of its docstring,
for every constant its value; and the one patch point of the extension object.  Needs the built
extension, not a GPU.

The tables were written down from the commit before ``ops/kernels.py`` was split by kernel
family and are never regenerated from the code under test: a name lost in a move, a changed
default or keyword, a dropped docstring or a copy of a name that is no longer the same object
fails here, not in a caller.  Two differences from that commit are deliberate and listed:
``DROPPED`` (what the old ``import *`` leaked) and ``ADDED`` (the by-format entry points).

Shorthand in the tables (expanded by ``_sig``): ``Tensor`` = 'torch.Tensor', ``Tensor?`` =
'Optional[torch.Tensor]'."""
import inspect
import os
import re

import mipipe  # noqa: F401
from mipipe import ops


def _sig(s):
    return re.sub(r"(?<![\w.\[])Tensor(\?)?", lambda m: "'Optional[torch.Tensor]'" if m.group(1) else "'torch.Tensor'", s)


_QLIN = ("scale: Tensor, bias: Tensor? = None, act: 'str' = 'none', residual: Tensor? = None, out: Tensor? = None, ")
_PAIR = "'Tuple[torch.Tensor, torch.Tensor]'"

# name -> (signature, first docstring line or None)
FUNCTIONS = {
    "act_bwd": ("(dg: Tensor, a: Tensor, act: 'str', dbias: Tensor? = None, p_drop: 'float' = 0.0, seed: 'int' = 0, "
                "out=None, saved: 'str' = 'pre')",
                "dA = dG * act'(.) (dropout mask regenerated from (seed, element index)), plus the"),
    "act_fwd": ("(a: Tensor, act: 'str', p_drop: 'float' = 0.0, seed: 'int' = 0, out=None)", None),
    "adamw_": ("(p, g, m, v, w16, n_decay: 'int', lr: 'float', b1: 'float', b2: 'float', eps: 'float', wd: 'float', "
               "step: 'int', sumsq_buf=None, max_norm: 'float' = 0.0, grad_scale: 'float' = 1.0, zero_grad: 'bool' = True)",
               "Fused AdamW over flat f32 buffers; also refreshes the bf16 copy ``w16`` and zeroes g."),
    "attn_append": ("(q, k_cache, v_cache, base, counts, o, T: 'int', H: 'int', Hkv: 'int', D: 'int', "
                    "scale: 'Optional[float]' = None, splits: 'int' = 0, max_len: 'Optional[int]' = None)",
                    "Attention of ``T`` new tokens per sequence over its KV cache.  q/o: [B*T, H*D] row"),
    "attn_append_plan": ("(B: 'int', T: 'int', Hkv: 'int', rep: 'int', max_len: 'int') -> 'int'",
                         "Key splits :func:`attn_append` picks (``splits=0``) for ``B`` sequences x ``T`` new"),
    "attn_bwd": ("(q, k, v, o, do, lse, dq, dk, dv, B: 'int', Sq: 'int', Sk: 'int', H: 'int', Hkv: 'int', D: 'int', "
                 "causal: 'bool', scale: 'Optional[float]' = None, p_drop: 'float' = 0.0, seed: 'int' = 0, delta=None, "
                 "dbias: Tensor? = None, doc_start: Tensor? = None, doc_end: Tensor? = None)",
                 "Writes dq, dk, dv (token-major views like the inputs).  ``dbias`` (f32"),
    "attn_decode": ("(q, k_cache, v_cache, lens, o, H: 'int', Hkv: 'int', D: 'int', scale: 'Optional[float]' = None, "
                    "splits: 'int' = 0, max_len: 'Optional[int]' = None)",
                    "Attention of one new token per sequence over its KV cache.  q/o: [B, H*D] row views"),
    "attn_decode_plan": ("(B: 'int', Hkv: 'int', max_len: 'int') -> 'int'",
                         "Key splits :func:`attn_decode` picks (``splits=0``) for ``B`` sequences x ``Hkv`` KV"),
    "attn_fwd": ("(q, k, v, o, lse, B: 'int', Sq: 'int', Sk: 'int', H: 'int', Hkv: 'int', D: 'int', causal: 'bool', "
                 "scale: 'Optional[float]' = None, p_drop: 'float' = 0.0, seed: 'int' = 0, doc_start: Tensor? = None)",
                 "q/k/v/o: token-major 2-D views ([B*S, row_stride], head h at cols h*D).  lse: f32"),
    "attn_plan": ("(B: 'int', Sq: 'int', Sk: 'int', H: 'int', Hkv: 'int', D: 'int', qs: 'int', ks: 'int', vs: 'int', "
                  "os: 'int', causal: 'bool', drop: 'bool', env: 'Optional[dict]' = None) -> 'dict'",
                  "What the bf16 :func:`attn_fwd` / :func:`attn_bwd` launch for a problem with row strides"),
    "cast_f32_bf16": ("(src: Tensor, dst: Tensor)", None),
    "colsum": ("(x: Tensor, dbias: Tensor)", None),
    "dequant_w4": ("(q4: Tensor, scale: Tensor, out: Tensor? = None) -> Tensor",
                   "out [N, K] = (q * scale per group) rounded to out's dtype (bf16 on the GPU): the"),
    "dequant_w8": ("(q: Tensor, scale: Tensor, out: Tensor? = None) -> Tensor",
                   "out = (q * scale) rounded to out's dtype (bf16 on the GPU): the effective weight."),
    "doc_bounds": (f"(tokens: Tensor, eos: 'int') -> {_PAIR}",
                   "(doc_start, doc_end), int32 [B*S], of ``tokens`` (int64 [B, S]): position i starts a"),
    "embed_bwd": ("(idx: Tensor, dout: Tensor, dwte: Tensor, dwpe: Tensor?, S: 'int', pos_offset: 'int' = 0)", None),
    "embed_fwd": ("(idx: Tensor, wte: Tensor, wpe: Tensor?, S: 'int', pos_offset: 'int' = 0, out: Tensor? = None, "
                  "positions: Tensor? = None)",
                  "``positions`` (int32 [T] on wte's device): one token per sequence, row t at position"),
    "ext_available": ("() -> 'bool'", None),
    "gemv_plan": ("(N: 'int', K: 'int', wbytes: 'int', force_split: 'int' = 0) -> 'Tuple[int, int]'",
                  "(weight rows per workgroup, K-splits) of the skinny kernel for an [N, K] weight of"),
    "linear": ("(x: Tensor, w: Tensor, bias: Tensor? = None, act: 'str' = 'none', residual: Tensor? = None, "
               "out: Tensor? = None, aux: Tensor? = None, p_drop: 'float' = 0.0, seed: 'int' = 0)",
               "y = drop(act(x @ w^T + bias)) (+ residual).  x [T,K], w [N,K].  With an activation"),
    "linear_dw": ("(dy: Tensor, x: Tensor, dw: Tensor, alpha: 'float' = 1.0)",
                  "dw (f32 [N,K]) += alpha * dy^T @ x   (dy [T,N], x [T,K])."),
    "linear_dx": ("(dy: Tensor, w: Tensor, act_input: Tensor? = None, act: 'str' = 'none', out: Tensor? = None, "
                  "residual: Tensor? = None, wt: Tensor? = None, colsum: Tensor? = None, p_drop: 'float' = 0.0, "
                  "seed: 'int' = 0)",
                  "dx = dy @ w  (w [N,K]), optionally times act'(.) given by ``act_input`` -- what"),
    "linear_f32": ("(x: Tensor, w: Tensor, b: Tensor? = None) -> Tensor",
                   "F.linear for f32 CUDA tensors on the f32 MFMA GEMM (autograd-aware)."),
    "linear_skinny": ("(x: Tensor, w: Tensor, scale: Tensor? = None, bias: Tensor? = None, act: 'str' = 'none', "
                      "residual: Tensor? = None, out: Tensor? = None, force_split: 'int' = 0) -> Tensor",
                      "y = act(x @ What^T + bias) (+ residual) for at most 16 rows of x, streaming the weight"),
    "linear_skinny_w4": (f"(x: Tensor, q4: Tensor, {_QLIN}force_split: 'int' = 0) -> Tensor",
                         ":func:`linear_skinny` over int4g128 weights (:func:`quantize_w4`): ``q4`` uint8"),
    "linear_w4": (f"(x: Tensor, q4: Tensor, {_QLIN}scratch: Tensor? = None) -> Tensor",
                  ":func:`linear` over int4g128 weights, any number of rows.  Up to ``W8_SKINNY_MAX_M``"),
    "linear_w8": (f"(x: Tensor, q: Tensor, {_QLIN}scratch: Tensor? = None) -> Tensor",
                  ":func:`linear` over int8 weights ``q`` [N, K] with ``scale`` [N], any number of rows."),
    "load_ext": ("()", None),
    "mean": ("(x: Tensor) -> Tensor", "Mean of an f32 tensor as a 0-dim f32 tensor (GPU: one deterministic workgroup,"),
    "norm_bwd": ("(dy: Tensor, s: Tensor, w: Tensor, mean, rstd, kind: 'str' = 'layernorm', dres: Tensor? = None, "
                 "dw: Tensor? = None, dbias: Tensor? = None, p_drop: 'float' = 0.0, seed: 'int' = 0, ds=None, dbranch=None, "
                 "want_branch: 'bool' = False, colsum_dres: Tensor? = None, colsum_ds: Tensor? = None, "
                 "colsum_branch: Tensor? = None)",
                 "ds = d(norm input) (+ dres); dw/dbias (f32) accumulate.  Optionally also accumulates"),
    "norm_fwd": ("(x: Tensor, w: Tensor, bias: Tensor? = None, branch: Tensor? = None, kind: 'str' = 'layernorm', "
                 "eps: 'float' = 1e-05, p_drop: 'float' = 0.0, seed: 'int' = 0, y=None, s=None, mean=None, rstd=None)",
                 "s = x + dropout(branch) (if branch given); y = norm(s) * w (+ bias).  Returns (y, s, mean, rstd)."),
    "plain_gemm_choices": ("() -> 'dict'", '{"fwd|dx MxNxK": backend} of the plain GEMM shapes decided so far (bench JSON).'),
    "plan_wjobs": ("(jobs)", "Split a job list into ``(small, long, rest)``: ``small`` -- lists of <= 8 short-token"),
    "quantize_w4": (f"(w: Tensor) -> {_PAIR}",
                    "Symmetric 4-bit quantisation of a 2-D weight ``w [N, K]`` (bf16 or f32) with one scale"),
    "quantize_w8": (f"(w: Tensor) -> {_PAIR}",
                    "Symmetric per-output-row int8 quantisation of a 2-D weight ``w [N, K]`` (bf16 or f32):"),
    "rope_": ("(qkv: Tensor, cos: Tensor, sin: Tensor, S: 'int', H: 'int', Hkv: 'int', Dh: 'int', pos_offset: 'int' = 0, "
              "inverse: 'bool' = False)",
              "In-place rotate-half RoPE on the q and k heads of a packed [T, (H+2Hkv)*Dh] buffer."),
    "rope_kv_append": ("(qkv: Tensor, cos: Tensor?, sin: Tensor?, k_cache: Tensor, v_cache: Tensor, pos: Tensor, "
                       "active: Tensor?, H: 'int', Hkv: 'int', Dh: 'int', rope: 'bool' = True, T: 'int' = 1, "
                       "counts: Tensor? = None)",
                       "``T`` new tokens per sequence (default one).  qkv: packed [B*T, (H + 2 Hkv) * Dh] rows,"),
    "rope_tables": (f"(S: 'int', Dh: 'int', theta: 'float', device) -> {_PAIR}", None),
    "run_wjobs": ("(jobs) -> 'None'",
                  "Run a list of weight-gradient jobs (:class:`DW` and :class:`ColSum` objects and plain"),
    "sample": ("(logits: Tensor, vocab: 'int', u: Tensor, temperature: 'float' = 0.0, top_k: 'int' = 0, "
               "top_p: 'float' = 1.0, done: Tensor? = None, stop_token: 'int' = -1, pad_token: 'int' = 0, "
               "out: Tensor? = None) -> Tensor",
               "One token id per row of ``logits`` [B, Vp] (bf16 or f32 rows, any row stride) over the"),
    "set_dropout_step": ("(step: 'int', device: 'Optional[torch.device]' = None) -> 'None'",
                         "Set the training-step counter every dropout kernel mixes into its seed (device"),
    "sumsq": ("(g: Tensor, out: Tensor)", None),
    "swiglu_bwd": ("(gu: Tensor, dy: Tensor, out=None)", None),
    "swiglu_fwd": ("(gu: Tensor, out=None)", None),
    "transpose": ("(x: Tensor, out: Tensor? = None) -> Tensor",
                  "out = x^T for a 2-D bf16 matrix (row-contiguous views allowed)."),
    "use_f32_kernels": ("(module: 'torch.nn.Module', on: 'bool' = True) -> 'int'",
                        "Route an f32 module's linears and attention projections to the f32 MFMA GEMM by"),
    "xent_fwd_bwd": ("(logits: Tensor, target: Tensor, vocab: 'int', grad_scale: 'float', ignore_index: 'int' = -100, "
                     "write_grad: 'bool' = True, loss: Tensor? = None)",
                     "Per-row CE loss (f32 [T]); if write_grad, logits are overwritten IN PLACE by"),
    "zero_": ("(t: Tensor) -> Tensor", "t <- 0 (GPU: hipMemsetAsync on the current stream instead of an ATen fill kernel)."),
}

CLASSES = {
    "ColSum": ("(x: Tensor, dbias: Tensor)",
               "A bias-gradient job ``dbias (f32) += column sums of x`` kept as data like :class:`DW`:"),
    "DW": ("(dy: Tensor, x: Tensor, dw: Tensor, alpha: 'float' = 1.0)",
           "A weight-gradient job ``dw (f32) += alpha * dy^T x`` kept as data, so that"),
    "F32Linear": ("(in_features: int, out_features: int, bias: bool = True, device=None, dtype=None) -> None",
                  "``nn.Linear`` whose f32 GPU forward/backward run on :func:`linear_f32` (other dtypes"),
    "F32MultiheadAttention": ("(embed_dim, num_heads, dropout=0.0, bias=True, add_bias_kv=False, add_zero_attn=False, "
                              "kdim=None, vdim=None, batch_first=False, device=None, dtype=None) -> None",
                              "``nn.MultiheadAttention`` whose input / output projections run on :func:`linear_f32`"),
}

# GEMM_BACKEND and GEMM_V: the defaults; MIPIPE_GEMM / MIPIPE_GEMM_V set them at import
CONSTANTS = {
    "ACT": {"none": 0, "gelu_tanh": 1, "gelu": 1, "relu": 2},
    "EPI_NONE": 0, "EPI_BIAS": 1, "EPI_BIAS_GELU": 2, "EPI_BIAS_RELU": 3, "EPI_BIAS_RES": 4, "EPI_RES": 5, "EPI_DGELU": 6,
    "EPI_DRELU": 7,
    "F32_NONE": 0, "F32_BIAS": 1, "F32_BIAS_RELU": 2, "F32_RES": 3, "F32_BIAS_RES": 4, "F32_DRELU": 5,
    "GEMM_BACKEND": os.environ.get("MIPIPE_GEMM", "hip"), "GEMM_V": int(os.environ.get("MIPIPE_GEMM_V", "2")),
    "LOG2E": 1.4426950408889634, "SKINNY_MAX_M": 16, "W8_SKINNY_MAX_M": 16, "W4_GROUP": 128,
}

# visible in ``ops`` before the split only because ``from .kernels import *`` had no ``__all__``; nothing used them
DROPPED = {"os", "math", "torch", "importlib", "Optional", "Tuple", "annotations"}
# new with the split: the quantised linear layers by format name
ADDED = {"QUANT_FORMATS", "linear_q"}
# private names that tools and tests reach through the facade
FACADE_PRIVATE = ("_ext", "_gemm", "_gemm_f32", "_gpu", "_mha_projected", "_cpu_attn_drop")
FAMILIES = ("norm_loss_embed", "gemm", "gemm_f32", "wgrad", "quant", "elementwise_optim", "attention", "generate")


def _public(mod):
    """public names of a module, the modules of the ``ops`` package itself aside"""
    return {n for n in dir(mod) if not n.startswith("_")
            and not (inspect.ismodule(getattr(mod, n)) and getattr(mod, n).__name__.startswith(ops.__name__ + "."))}


def test_counts_of_the_table():
    assert (len(FUNCTIONS), len(CLASSES), len(CONSTANTS)) == (48, 4, 21)


def test_public_names():
    table = set(FUNCTIONS) | set(CLASSES) | set(CONSTANTS)
    assert not table & (DROPPED | ADDED)
    have = _public(ops)
    assert have - ADDED == table, (sorted(have - ADDED - table), sorted(table - have))
    assert ADDED <= have
    if hasattr(ops, "__all__"):
        assert set(ops.__all__) == table | ADDED


def test_signatures_docstrings_and_values():
    for name, (sig, doc) in {**FUNCTIONS, **CLASSES}.items():
        obj = getattr(ops, name)
        assert inspect.isclass(obj) == (name in CLASSES), name
        assert str(inspect.signature(obj)) == _sig(sig), name
        first = obj.__doc__.strip().splitlines()[0] if obj.__doc__ else None
        assert first == doc, name
    for name, value in CONSTANTS.items():
        got = getattr(ops, name)
        assert type(got) is type(value) and got == value, name


def test_facade_holds_the_same_objects():
    K = ops.kernels
    for name in set(FUNCTIONS) | set(CLASSES) | set(CONSTANTS) | ADDED:
        assert getattr(K, name) is getattr(ops, name), name
    assert _public(K) == _public(ops)
    owners = {n: m for m in (ops._base,) + tuple(getattr(ops, f) for f in FAMILIES) for n in vars(m)}
    for name in FACADE_PRIVATE:
        assert getattr(K, name) is getattr(owners[name], name), name


def test_one_patch_point_for_the_extension(monkeypatch):
    """Whatever stands in ``_base._EXT`` is what every family module and the facade call."""
    sentinel = object()
    monkeypatch.setattr(ops._base, "_EXT", sentinel)
    assert ops.load_ext() is sentinel and ops.kernels.load_ext() is sentinel and ops.ext_available()
    for mod in (ops.kernels, ops._base) + tuple(getattr(ops, f) for f in FAMILIES):
        assert mod._ext() is sentinel, mod.__name__
    monkeypatch.undo()
    assert ops.kernels._ext() is ops.load_ext() is not sentinel


def test_switches_live_in_one_module():
    """A switch is a module global of exactly one family module (the facade and ``ops`` hold
    import-time copies of the two public ones, for reading)."""
    where = {"GEMM_BACKEND": "gemm", "GEMM_V": "gemm", "_WGRAD_GROUP": "wgrad", "_WGRAD_GROUP3": "wgrad",
             "_GROUP3_MIN_T": "wgrad"}
    for name, owner in where.items():
        have = [f for f in ("_base",) + FAMILIES if name in vars(getattr(ops, f))]
        assert have == [owner], name
