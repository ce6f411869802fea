"""The Python-visible surface of the built extension ``_C`` (csrc/bindings/*.cpp, the RCCL engine
and the stage runner register into one module): the set of public names, and for every function
the signature line pybind11 writes into ``__doc__`` (argument names, annotated types, defaults,
return type) and the docstring behind it.  Needs the built extension, not a GPU.

The tables were written down from the build of the commit before the bindings were split by
kernel family and are never regenerated from the code under test: a missing or extra name, a
renamed keyword, a changed default or a dropped docstring fails here, not in a caller.

Shorthand in the tables (expanded by ``_sig``): ``Tensor`` = torch.Tensor, ``Tensor?`` =
torch.Tensor | None, ``Int`` / ``Float`` = typing.SupportsInt / typing.SupportsFloat, ``Seq[`` =
collections.abc.Sequence[, ``Env?`` = collections.abc.Mapping[str, str] | None, ``Self`` = the class."""
import re

import mipipe  # noqa: F401
from mipipe.ops import kernels as K


def _sig(s, cls=""):
    for short, full in (("Tensor?", "torch.Tensor | None"), ("Tensor", "torch.Tensor"), ("Int", "typing.SupportsInt"),
                        ("Float", "typing.SupportsFloat"), ("Seq[", "collections.abc.Sequence["),
                        ("Env?", "collections.abc.Mapping[str, str] | None"), ("Self", "mipipe._C." + cls)):
        s = re.sub(r"(?<![\w.])" + re.escape(short), full, s)
    return s


def _args(n, types):
    """'arg0: <t0>, arg1: <t1>, ...' of an unnamed-argument binding; types: one shorthand per argument."""
    types = types.split()
    assert len(types) == n
    return ", ".join(f"arg{i}: {t}" for i, t in enumerate(types))


# name -> (signature without the name, docstring or None)
FUNCTIONS = {
    "act_bwd": (f"({_args(7, 'Tensor Tensor Tensor Tensor? Int Float Int')}) -> None", None),
    "act_fwd": (f"({_args(5, 'Tensor Tensor Int Float Int')}) -> None", None),
    "adamw": ("(" + _args(16, "Tensor Tensor Tensor Tensor Tensor? Int Float Float Float Float Float Int Tensor? Float "
                          "Float bool") + ") -> None", None),
    "attn_append": ("(q: Tensor, k_cache: Tensor, v_cache: Tensor, base: Tensor, counts: Tensor?, o: Tensor, T: Int, "
                    "H: Int, Hkv: Int, D: Int, max_len: Int, scale: Float, splits: Int = 0) -> int", None),
    "attn_append_plan": (f"({_args(5, 'Int Int Int Int Int')}) -> int",
                         "key splits the append attention picks for B sequences x T tokens x Hkv KV heads of rep "
                         "query heads over max_len keys"),
    "attn_bwd": ("(" + _args(21, "Tensor Tensor Tensor Tensor Tensor Tensor Tensor Tensor Tensor Tensor Int Int Int Int "
                             "Int Int bool Float Float Int Tensor?") + ") -> None", None),
    "attn_decode": ("(q: Tensor, k_cache: Tensor, v_cache: Tensor, lens: Tensor, o: Tensor, H: Int, Hkv: Int, D: Int, "
                    "max_len: Int, scale: Float, splits: Int = 0) -> int", None),
    "attn_decode_plan": (f"({_args(3, 'Int Int Int')}) -> int",
                         "key splits the decode attention picks for B sequences x Hkv KV heads over max_len keys"),
    "attn_doc_bwd": ("(" + _args(20, "Tensor Tensor Tensor Tensor Tensor Tensor Tensor Tensor Tensor Tensor Tensor "
                                 "Tensor Int Int Int Int Int bool Float Float") + ") -> None", None),
    "attn_doc_fwd": ("(" + _args(14, "Tensor Tensor Tensor Tensor Tensor Tensor Int Int Int Int Int bool Float Float")
                     + ") -> None", None),
    "attn_fwd": ("(" + _args(15, "Tensor Tensor Tensor Tensor Tensor Int Int Int Int Int Int bool Float Float Int")
                 + ") -> None", None),
    "attn_plan": ("(B: Int, Sq: Int, Sk: Int, H: Int, Hkv: Int, D: Int, qs: Int, ks: Int, vs: Int, os: Int, "
                  "causal: bool, drop: bool, env: Env? = None) -> dict",
                  "kernels, grids and LDS bytes the bf16 attention launches; env: the MIPIPE_ATTN_* switches as a "
                  "dict over their defaults instead of the process environment"),
    "cast_f32_bf16": (f"({_args(2, 'Tensor Tensor')}) -> None", None),
    "colsum": (f"({_args(2, 'Tensor Tensor')}) -> None", None),
    "comm_stream": ("(device: Int, slot: Int) -> int", None),
    "create_stream": ("(device: Int, priority: Int = 0) -> int", None),
    "dequant_w8": (f"({_args(3, 'Tensor Tensor Tensor')}) -> None", None),
    "doc_bounds": (f"({_args(2, 'Tensor Int')}) -> list[torch.Tensor]", None),
    "embed_bwd": (f"({_args(6, 'Tensor Tensor Tensor Tensor? Int Int')}) -> None", None),
    "embed_fwd": (f"({_args(6, 'Tensor Tensor Tensor? Tensor Int Int')}) -> None", None),
    "embed_pos": (f"({_args(5, 'Tensor Tensor Tensor Tensor? Tensor')}) -> None", None),
    "gemm": (f"({_args(11, 'Tensor Tensor Tensor Tensor? Tensor? Tensor? bool bool Int bool Float')}) -> None", None),
    "gemm2": ("(A: Tensor, B: Tensor, C: Tensor, bias: Tensor?, residual: Tensor?, aux: Tensor?, transA: bool, "
              "transB: bool, epilogue: Int, accum: bool, alpha: Float, force_cfg: Int, colsum: Tensor?, "
              "p_drop: Float = 0.0, seed: Int = 0) -> int", None),
    "gemm2_has_probe_engines": ("() -> bool", None),
    "gemm2_plan": ("(M: Int, N: Int, K: Int, transA: bool, transB: bool, accum: bool, force_cfg: Int, "
                   "env: Env? = None) -> tuple[int, int]",
                   "engine config + split-K factor the v2 GEMM picks (14: stream-K gemm7); env: the MIPIPE_* planner "
                   "switches as a dict over their defaults instead of the process environment"),
    "gemm_dw_grouped": ("(dy: Seq[Tensor], x: Seq[Tensor], C: Seq[Tensor], alpha: Float = 1.0, split: Int = 0) -> int",
                        None),
    "gemm_f32": (f"({_args(6, 'Tensor Tensor Tensor Tensor? Float bool')}) -> int", None),
    "gemm_f32_ex": ("(A: Tensor, B: Tensor, C: Tensor, bias: Tensor?, R: Tensor?, X: Tensor?, epi: Int = 0, "
                    "alpha: Float = 1.0, accumulate: bool = False, p_drop: Float = 0.0, seed: Int = 0, "
                    "force_ks: Int = 0) -> int", None),
    "gemm_f32_plan": (f"({_args(4, 'Int Int Int Int')}) -> tuple[bool, int, int, int]",
                      "what gemm_f32_ex will run: (128x128 engine, split-K factor, stream-K workgroups, K-tile pairs "
                      "per workgroup)"),
    "gemm_f32_set_lanes": (f"({_args(1, 'Int')}) -> int", None),
    "gemm_tt_grouped": ("(dy: Seq[Tensor], x: Seq[Tensor], C: Seq[Tensor], alpha: Float = 1.0) -> None", None),
    "gemv_plan": ("(N: Int, K: Int, wbytes: Int, force_split: Int = 0) -> tuple[int, int]",
                  "(weight rows per workgroup, K-splits = waves per workgroup) of the skinny-M kernel"),
    "gemv_skinny": ("(x: Tensor, w: Tensor, scale: Tensor?, y: Tensor, bias: Tensor?, residual: Tensor?, "
                    "gelu: bool = False, force_split: Int = 0) -> None", None),
    "lane_merge": ("(g0: Tensor, lanes: Seq[Tensor], sumsq: Tensor? = None) -> None", None),
    "norm_bwd": ("(" + _args(15, "bool Tensor Tensor Tensor Tensor? Tensor Tensor? Tensor Tensor? Tensor Tensor? Float "
                             "Int Tensor? Tensor?") + ") -> int", None),
    "norm_fwd": ("(" + _args(12, "bool Tensor Tensor? Tensor Tensor? Tensor? Tensor Tensor? Tensor Float Float Int")
                 + ") -> None", None),
    "probe_clock_khz": ("() -> int", None),
    "probe_set": ("(flag: Tensor, value: Int, setter: Int = 0) -> None", None),
    "probe_spin": ("(flag: Tensor, expect: Int, timeout_us: Int, result: Tensor, waiter: Int = 0) -> None", None),
    "rope": (f"({_args(9, 'Tensor Tensor Tensor Int Int Int Int Int bool')}) -> None", None),
    "rope_kv_append": ("(qkv: Tensor, cos: Tensor?, sin: Tensor?, k_cache: Tensor, v_cache: Tensor, pos: Tensor, "
                       "active: Tensor?, H: Int, Hkv: Int, Dh: Int, rope: bool, T: Int = 1, counts: Tensor? = None) "
                       "-> None", None),
    "sample": (f"({_args(10, 'Tensor Int Tensor Float Int Float Tensor? Int Int Tensor')}) -> None", None),
    "scaled_sum": (f"({_args(3, 'Tensor Float Tensor')}) -> None", None),
    "set_dropout_step": (f"({_args(1, 'Int')}) -> None", None),
    "sumsq": (f"({_args(2, 'Tensor Tensor')}) -> None", None),
    "swiglu_bwd": (f"({_args(3, 'Tensor Tensor Tensor')}) -> None", None),
    "swiglu_fwd": (f"({_args(2, 'Tensor Tensor')}) -> None", None),
    "transpose": (f"({_args(2, 'Tensor Tensor')}) -> None", None),
    "transpose_batched": (f"({_args(5, 'Tensor Tensor Tensor Tensor Int')}) -> None", None),
    "xent": (f"({_args(7, 'Tensor Tensor Tensor Int Float Int bool')}) -> None", None),
    "zero_": (f"({_args(1, 'Tensor')}) -> None", None),
}

_POST = "Seq[tuple[Tensor, Int]]"
_TAPE = "Seq[tuple[Int, Int, Int, Int]]"
# class -> member -> signature without the name (None: a property)
CLASSES = {
    "RcclEngine": {
        "__init__": "(self: Self, unique_ids: bytes, nranks: Int, rank: Int, device: Int, slots: Seq[Int]) -> None",
        "abort": "(self: Self) -> None", "async_error": "(self: Self) -> str", "channels": None,
        "close": "(self: Self) -> None",
        "coll": "(self: Self, channel: Int, op: Int, send: Tensor, recv: Tensor) -> int",
        "id_bytes": "() -> int", "issued": "(self: Self) -> int", "load": "(arg0: str) -> None", "nranks": None,
        "post": f"(self: Self, channel: Int, sends: {_POST}, recvs: {_POST}) -> int",
        "progress": "(self: Self) -> list", "query": "(self: Self, arg0: Int) -> bool", "rank": None,
        "release": "(self: Self, arg0: Int) -> None", "slot": "(self: Self, arg0: Int) -> int",
        "stream_handle": "(self: Self, arg0: Int) -> int", "synchronize": "(self: Self) -> None",
        "unique_id": "() -> bytes", "wait": "(self: Self, arg0: Int) -> None",
        "wait_keep": "(self: Self, arg0: Int) -> None",
    },
    "StageRunner": {
        "__init__": "(self: Self, device: Int) -> None",
        "add_call": "(self: Self, arg0: collections.abc.Callable) -> None",
        "add_coll": "(self: Self, arg0: object, arg1: Int, arg2: Int, arg3: Int, arg4: Int, arg5: Int, arg6: Int) -> int",
        "add_copy": "(self: Self, dst: Int, src: Int, nbytes: Int, stream: Int = 0) -> None",
        "add_graph": "(self: Self, graph_exec: Int, label: str = '', stream: Int = 0) -> None",
        "add_post": f"(self: Self, arg0: object, arg1: Int, arg2: {_TAPE}, arg3: {_TAPE}) -> int",
        "add_sync": "(self: Self, waiter: Int, signal: Int) -> None",
        "add_wait": "(self: Self, slot: Int, stream: Int = 0) -> None",
        "channels": "(self: Self) -> list[int]", "collectives": "(self: Self) -> list[tuple[int, int]]",
        "kinds": "(self: Self) -> list[int]", "recv_early": "(self: Self) -> bool", "run": "(self: Self) -> None",
        "runs": None, "set_profile": "(self: Self, arg0: bool) -> None",
        "set_recv_early": "(self: Self, arg0: bool) -> None", "size": None,
        "timeline": "(self: Self) -> tuple[list[tuple[str, float, float]], float]",
    },
}

VALUES = {"COMM_STREAM_SLOTS": 3}


def _ext():
    ext = K.load_ext()
    assert ext is not None, "the extension is not built (python tools/build_ext.py)"
    return ext


def _public(obj):
    return {n for n in dir(obj) if not n.startswith("_")}


def test_public_names():
    assert _public(_ext()) == set(FUNCTIONS) | set(CLASSES) | set(VALUES)
    for name, value in VALUES.items():
        assert getattr(_ext(), name) == value


def test_function_signatures_and_docstrings():
    for name, (sig, doc) in FUNCTIONS.items():
        got = getattr(_ext(), name).__doc__
        want = name + _sig(sig) + "\n" + (f"\n{doc}\n" if doc else "")
        assert got == want, name


def test_class_members():
    for cls, members in CLASSES.items():
        c = getattr(_ext(), cls)
        assert isinstance(c, type)
        assert _public(c) | {"__init__"} == set(members), cls
        for name, sig in members.items():
            got = (getattr(c, name).__doc__ or "").strip()
            assert got == ("" if sig is None else name + _sig(sig, cls)), f"{cls}.{name}"
