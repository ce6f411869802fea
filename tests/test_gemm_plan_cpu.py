"""The bf16 GEMM planner (csrc/include/mp_gemm_plan.h plan_gemm: host code, runs without a GPU)
through the binding ``gemm2_plan(M, N, K, transA, transB, accum, force_cfg, env=None)``.

TABLE pins one row per rule of the planner and per MIPIPE_* switch.  Every expected value was
recorded from the build of the commit before the planner became a pure function (its switches
were read once per process there: one child process per environment), so the table holds the
planner to that behaviour, oddities included.  ``env`` gives the switches as a dict over their
defaults, which is what lets one process reach them."""
import os

import pytest

import mipipe  # noqa: F401
from mipipe.ops import kernels as K

NT, TN, NTR, TT = (False, False), (True, False), (False, True), (True, True)   # (transA, transB)

# (M, N, K, layout, accum, force_cfg, env) -> (cfg, split); a second expectation where the probes
# build (MP_PROBE_ENGINES) answers differently
TABLE = [
    # --- NT, bf16 output ---------------------------------------------------------------------
    (320, 192, 128, NT, 0, -1, {}, (12, 1), None),       # short problem: small engine, 32x32 (test_wrappers_dispatch)
    (320, 128, 192, NT, 0, -1, {}, (12, 1), None),       #   its dX (test_wrappers_dispatch)
    (1024, 768, 3072, NT, 0, -1, {}, (11, 1), None),     #   64x32 gives 256 workgroups
    (4096, 768, 768, NT, 0, -1, {}, (10, 1), None),      #   64x64 does
    (256, 768, 16384, NT, 0, -1, {}, (2, 8), None),      # short but K > 4096: the big split-K plan
    (16384, 3072, 768, NT, 0, -1, {}, (5, 1), None),     # 256x256 tile -> ping-pong M16
    (16384, 768, 768, NT, 0, -1, {}, (5, 1), None),      # 256x192 tile, unsplit, >= 96 tiles -> ping-pong M16
    (6144, 768, 768, NT, 0, -1, {}, (2, 1), None),       # 72 tiles: the 2-stage tile stays
    (8192, 768, 3072, NT, 0, -1, {}, (1, 2), None),      # split-K plan keeps its 2-stage tile
    (2304, 4096, 16384, NT, 0, -1, {}, (5, 5), None),    # 256x256 with split-K: ping-pong into slabs
    # --- NT, f32 accumulate ------------------------------------------------------------------
    (64, 128, 4160, NT, 1, -1, {}, (2, 13), None),       # 65 K-tiles in 13 splits (test_wrappers_dispatch)
    (320, 192, 128, NT, 1, -1, {}, (2, 1), None),        # never the small engine
    (16384, 768, 768, NT, 1, -1, {}, (5, 1), None),
    # --- MIPIPE_GEMM3 / MIPIPE_GEMM_M16 ------------------------------------------------------
    (16384, 3072, 768, NT, 0, -1, {"MIPIPE_GEMM3": "0"}, (0, 1), None),
    (16384, 768, 768, NT, 0, -1, {"MIPIPE_GEMM3": "0"}, (1, 1), None),
    (16384, 3072, 768, NT, 0, -1, {"MIPIPE_GEMM_M16": "0"}, (4, 1), None),   # the 32x32x16 build
    (16384, 768, 768, NT, 0, -1, {"MIPIPE_GEMM_M16": "0"}, (1, 1), None),    #   takes no other tile's problems
    # --- opt-in engines where ping-pong M16 would run unsplit --------------------------------
    (32768, 768, 768, NT, 0, -1, {"MIPIPE_GEMM6": "1"}, (9, 1), None),       # 1.5 rounds of 256x256: gemm6
    (16384, 768, 768, NT, 0, -1, {"MIPIPE_GEMM6": "1"}, (5, 1), None),       #   one round: no
    (65536, 768, 768, NT, 0, -1, {"MIPIPE_GEMM6": "1"}, (5, 1), None),       #   whole rounds: no
    (16384, 768, 768, NT, 0, -1, {"MIPIPE_GEMM8": "1"}, (15, 1), None),
    (16384, 768, 768, NT, 1, -1, {"MIPIPE_GEMM8": "1"}, (15, 1), None),      #   f32 accumulate too
    (16384, 768, 768, NT, 0, -1, {"MIPIPE_GEMM8": "auto"}, (15, 1), None),   # by its round model
    (65536, 768, 768, NT, 0, -1, {"MIPIPE_GEMM8": "auto"}, (5, 1), None),
    (16384, 768, 768, NT, 1, -1, {"MIPIPE_GEMM8": "auto"}, (5, 1), None),    #   bf16 outputs only
    (16384, 768, 768, NT, 0, -1, {"MIPIPE_GEMM5": "1"}, (5, 1), (8, 1)),     # probe builds only
    (8192, 768, 768, NT, 0, -1, {"MIPIPE_GEMM_SK": "1"}, (5, 1), (14, 1)),   # probe builds only: a partial round
    (65536, 768, 768, NT, 0, -1, {"MIPIPE_GEMM_SK": "1"}, (5, 1), None),     #   whole rounds: no
    (4096, 768, 768, NT, 0, -1, {"MIPIPE_GEMM_SK": "1"}, (10, 1), None),     #   the small engine keeps its problems
    # --- MIPIPE_GEMM_SMALL / MIPIPE_GEMMS_MINWG ----------------------------------------------
    (320, 192, 128, NT, 0, -1, {"MIPIPE_GEMM_SMALL": "0"}, (2, 1), None),
    (192, 128, 320, TT, 1, -1, {"MIPIPE_GEMM_SMALL": "0"}, (2, 1), None),
    (320, 192, 128, NT, 0, -1, {"MIPIPE_GEMMS_MINWG": "8"}, (10, 1), None),
    (320, 192, 128, NT, 0, -1, {"MIPIPE_GEMMS_MINWG": "64"}, (12, 1), None),
    (320, 192, 128, NT, 0, -1, {"MIPIPE_GEMMS_MINWG": "0"}, (12, 1), None),  # non-positive: the default 256
    # --- TT (dW) -----------------------------------------------------------------------------
    (192, 128, 320, TT, 1, -1, {}, (13, 1), None),       # short: small TT engine (test_wrappers_dispatch)
    (768, 768, 4160, TT, 1, -1, {}, (2, 13), None),      # short but K > 4096
    (768, 3072, 16384, TT, 1, -1, {}, (6, 7), None),     # 256x256 tile -> ping-pong TT
    (768, 768, 65536, TT, 1, -1, {}, (6, 28), None),
    (768, 3072, 16384, TT, 1, -1, {"MIPIPE_GEMM3T": "0"}, (0, 7), None),
    (768, 3072, 16384, TT, 1, -1, {"MIPIPE_DW_MAXSPLIT": "4"}, (2, 3), None),
    (768, 3072, 16384, TT, 1, -1, {"MIPIPE_DW_MAXSPLIT": "-3"}, (6, 7), None),   # non-positive: the default 32
    (768, 3072, 16384, TT, 0, -1, {}, (0, 7), None),     # bf16 output: 2-stage tile, split-K slabs
    (192, 128, 320, TT, 0, -1, {}, (2, 1), None),
    # --- mixed layouts -----------------------------------------------------------------------
    (768, 3072, 16384, TN, 1, -1, {}, (0, 7), None),
    (768, 3072, 16384, TN, 0, -1, {}, (0, 1), None),     # bf16 output: no split-K
    (256, 768, 16384, NTR, 1, -1, {}, (2, 32), None),
    (256, 768, 16384, NTR, 0, -1, {}, (2, 1), None),
    # --- switches that only launchers read: the plan does not move ---------------------------
    (16384, 768, 768, NT, 0, -1, {"MIPIPE_GEMM4": "1"}, (5, 1), None),
    (768, 3072, 16384, TT, 1, -1, {"MIPIPE_GEMM_M16T": "1"}, (6, 7), None),
    (768, 3072, 16384, TT, 1, -1, {"MIPIPE_DW_GROUP_SPLIT": "3"}, (6, 7), None),
    (8192, 768, 768, NT, 0, -1, {"MIPIPE_GEMM7_S": "2"}, (5, 1), None),
    # --- forced configurations ---------------------------------------------------------------
    (4096, 768, 768, NT, 0, 0, {}, (0, 1), None),        # a forced tile is not promoted to ping-pong
    (256, 768, 16384, NT, 0, 2, {}, (2, 8), None),       #   and keeps the model's split
    (256, 768, 16384, TN, 0, 2, {}, (2, 1), None),       #   except mixed-layout bf16 outputs
    (4096, 768, 768, TT, 1, 1, {}, (2, 2), None),        # 256x192 needs K-contiguous operands
    (4096, 768, 768, NT, 0, 4, {}, (4, 1), None),
    (4096, 768, 768, TT, 1, 5, {}, (0, 2), None),        # ping-pong NT builds: NT only
    (4096, 768, 768, NT, 0, 6, {}, (0, 1), None),        # ping-pong TT: TT f32 accumulate only
    (768, 3072, 16384, TT, 1, 6, {}, (6, 7), None),
    (768, 3072, 16384, TT, 0, 6, {}, (0, 7), None),
    (4096, 768, 768, NT, 0, 9, {}, (9, 1), None),
    (4096, 768, 768, TT, 1, 9, {}, (0, 1), None),
    (4096, 768, 768, NT, 0, 11, {}, (11, 1), None),
    (4096, 768, 768, NT, 0, 12, {"MIPIPE_GEMM_SMALL": "0"}, (0, 1), None),   # the placeholder 256x256 tile survives
    (4096, 768, 768, TT, 1, 12, {}, (0, 2), None),       #   here too
    (192, 128, 16384, TT, 1, 13, {}, (13, 1), None),
    (4096, 768, 768, NT, 0, 13, {}, (10, 1), None),      # odd: the unforced short-problem rule answers
    (32768, 768, 16384, NT, 0, 13, {}, (0, 1), None),    # odd: the placeholder
    (32768, 768, 768, NT, 0, 15, {}, (15, 1), None),
    (32768, 768, 768, NT, 0, 16, {}, (16, 1), None),
    (32768, 768, 16384, TT, 1, 15, {}, (0, 2), None),
    (8192, 768, 768, NT, 0, 14, {}, (-1, 1), (14, 1)),   # probe engines: refused unless built
    (65536, 768, 768, NT, 0, 14, {}, (-1, 1), (0, 1)),   #   whole rounds: plan7 declines, the placeholder
    (2048, 768, 768, NT, 0, 14, {}, (-1, 1), (10, 1)),
    (8192, 768, 768, NT, 0, 7, {}, (-1, 1), (7, 1)),
    (8192, 768, 768, NT, 0, 8, {}, (-1, 1), (8, 1)),
    (8192, 768, 768, NT, 0, 104, {}, (-1, 1), (7, 1)),
]


@pytest.fixture(scope="module")
def ext():
    e = K.load_ext()
    if e is None or not hasattr(e, "gemm2_plan"):
        pytest.skip("extension not built")
    return e


def test_plan_table(ext):
    probes = ext.gemm2_has_probe_engines()
    bad = []
    for M, N, Kd, (ta, tb), acc, force, env, want, want_probes in TABLE:
        if probes and want_probes is not None:
            want = want_probes
        got = ext.gemm2_plan(M, N, Kd, ta, tb, bool(acc), force, env=env)
        if tuple(got) != want:
            bad.append(((M, N, Kd, ta, tb, acc, force, env), tuple(got), want))
    assert not bad, bad


def test_plan_env_names(ext):
    with pytest.raises(Exception, match="MIPIPE_GEMM9"):
        ext.gemm2_plan(320, 192, 128, False, False, False, -1, env={"MIPIPE_GEMM9": "1"})
    with pytest.raises(Exception, match="not a planner switch"):
        ext.gemm2_plan(320, 192, 128, False, False, False, -1, env={"MIPIPE_GEMM": "hip"})


def test_plan_default_env_is_process_env(ext):
    if any(k.startswith(("MIPIPE_GEMM", "MIPIPE_DW")) for k in os.environ):
        pytest.skip("a planner switch is set in this process")
    for M, N, Kd, (ta, tb), acc, force, env, _, _ in TABLE:
        args = (M, N, Kd, ta, tb, bool(acc), force)
        assert ext.gemm2_plan(*args) == ext.gemm2_plan(*args, env={}) == ext.gemm2_plan(*args, env=None), args


def test_gemm_planner_split_tail_is_opt_in(monkeypatch):
    """mp_gemm_plan.h plan_gemm (host code, runs without a GPU): the split-tail engine (cfg
    14, opt-in) accepts NT grids that are not whole rounds of 256 CUs -- a pipeline rank's
    8K-32K-token microbatches -- and never whole rounds (64K tokens, N = 768: 768 tiles = 3
    rounds), dW (TT, f32 accumulate) or short-token grids."""
    from mipipe.ops import kernels as K
    e = K.load_ext()
    if e is None or not hasattr(e, "gemm2_plan"):
        pytest.skip("extension not built")
    # default: off (a measured null, mp_gemm_plan.h); force_cfg 14 plans it where it applies
    assert e.gemm2_plan(8192, 768, 768, False, False, False, -1)[0] != 14
    if not e.gemm2_has_probe_engines():
        # the default _C.so does not carry the probe engines (tools/build_ext.py --variant
        # probes -D MP_PROBE_ENGINES): the planner refuses to plan one it cannot launch
        assert e.gemm2_plan(8192, 768, 768, False, False, False, 14)[0] == -1
        return
    assert e.gemm2_plan(8192, 768, 768, False, False, False, 14)[0] == 14
    plan = lambda M, N, Kd, ta=False, tb=False, acc=False: e.gemm2_plan(M, N, Kd, ta, tb, acc, 14)[0]  # noqa: E731
    for M, N, Kd in ((8192, 768, 768), (8192, 768, 3072), (32768, 768, 3072), (32768, 768, 2304)):
        assert plan(M, N, Kd) == 14, (M, N, Kd)
    # whole rounds, or a tail too wide to split into chunks (16K x 768: 192 tiles)
    for M, N, Kd in ((65536, 768, 768), (65536, 768, 3072), (65536, 3072, 768), (16384, 768, 3072)):
        assert plan(M, N, Kd) != 14, (M, N, Kd)
    assert plan(2048, 768, 768) != 14                       # 24 tiles: below the split threshold
    assert plan(768, 3072, 32768, True, True, True) != 14    # dW
