"""The launch plan of the training attention (csrc/include/mp_attn_plan.h: host code, runs without
a GPU) through ``ops.attn_plan(B, Sq, Sk, H, Hkv, D, qs, ks, vs, os, causal, drop, env=None)``.

Two checks.  attn_refs.path() re-states the launch rules by hand; it labels the GPU edge cases
and chooses them ("the smallest shapes that reach each launcher branch"), so the plan must name
the kernels path() names for every one of them, and the rest of each label (pair count, role
blocks, key-split iterations) must match the planned grid and LDS size.  TABLE pins one row
per rule and per switch value with the kernel, grid and LDS bytes written out."""
import os
import re

import pytest

import mipipe  # noqa: F401
from mipipe import ops
from mipipe.ops import kernels as K

import attn_refs as R

LDS_MAX = 160 * 1024    # CDNA4: LDS per workgroup

BIG = R.BIG_STRIDE
V1 = R.CHILD_ENVS["v1"]

# (B, Sq, Sk, H, Hkv, D, causal, drop, (qs, ks, vs, os) or None for packed rows H*D / Hkv*D, env)
#   -> forward (kernel, grid, lds), backward [(kernel, grid, lds), ...]
C257 = (2, 257, 257, 3, 3, 64, True, False, None)      # causal, 3 query blocks = 2 pairs, B*H = 6
S64 = (2, 64, 64, 3, 3, 64, False, False, None)        # short non-causal
D_ROW = lambda D: (1, 129, 129, 2, 2, D, True, False, None)   # noqa: E731
BIGROW = lambda qs, ks, vs, os: (1, 128, 128, 2, 2, 64, True, False, (qs, ks, vs, os))   # noqa: E731
FWD2, DQ3, DKDV3 = 32768, 65536, 67584                 # LDS bytes of the d_h 64 ring kernels
TABLE = [
    # --- d_h 64 defaults: forward v2, dQ v3, dK/dV v3; causal pairs the 128-row blocks -----------
    ((8, 1024, 1024, 12, 12, 64, True, False, None, {}),
     ("fwd2", (384, 1), FWD2), [("dq3", (384, 1), DQ3), ("dkdv3", (384, 1), DKDV3)]),
    ((8, 1024, 1024, 12, 12, 64, True, True, None, {}),        # dropout picks the instantiation only
     ("fwd2", (384, 1), FWD2), [("dq3", (384, 1), DQ3), ("dkdv3", (384, 1), DKDV3)]),
    ((8, 1024, 1024, 12, 12, 64, False, False, None, {}),      # non-causal: one block per workgroup
     ("fwd2", (768, 1), FWD2), [("dq3", (768, 1), DQ3), ("dkdv3", (768, 1), DKDV3)]),
    (C257 + ({},), ("fwd2", (12, 1), FWD2), [("dq3", (12, 1), DQ3), ("dkdv3", (12, 1), DKDV3)]),
    ((1, 257, 257, 8, 2, 64, True, False, None, {}),           # GQA: dK/dV runs per KV head
     ("fwd2", (16, 1), FWD2), [("dq3", (16, 1), DQ3), ("dkdv3", (4, 1), DKDV3)]),
    ((2, 100, 300, 3, 3, 64, False, False, None, {}),          # cross lengths: 1 query block, 3 key blocks
     ("ks2", (2, 6), 65536), [("dq3", (6, 1), DQ3), ("dkdv3", (18, 1), DKDV3)]),
    # --- MIPIPE_ATTN_FWD / BWD_DQ / BWD_DKDV -----------------------------------------------------
    (C257 + ({"MIPIPE_ATTN_FWD": "1"},), ("fwd1", (3, 6), 32768), [("dq3", (12, 1), DQ3), ("dkdv3", (12, 1), DKDV3)]),
    (C257 + ({"MIPIPE_ATTN_FWD": "2"},), ("fwd2", (12, 1), FWD2), [("dq3", (12, 1), DQ3), ("dkdv3", (12, 1), DKDV3)]),
    (C257 + ({"MIPIPE_ATTN_BWD_DQ": "1"},), ("fwd2", (12, 1), FWD2), [("dq1", (3, 6), 65536), ("dkdv3", (12, 1), DKDV3)]),
    (C257 + ({"MIPIPE_ATTN_BWD_DQ": "2"},), ("fwd2", (12, 1), FWD2), [("dq2", (3, 6), DQ3), ("dkdv3", (12, 1), DKDV3)]),
    (C257 + ({"MIPIPE_ATTN_BWD_DQ": "3"},), ("fwd2", (12, 1), FWD2), [("dq3", (12, 1), DQ3), ("dkdv3", (12, 1), DKDV3)]),
    (C257 + ({"MIPIPE_ATTN_BWD_DKDV": "1"},), ("fwd2", (12, 1), FWD2), [("dq3", (12, 1), DQ3), ("dkdv1", (3, 6), 67584)]),
    (C257 + ({"MIPIPE_ATTN_BWD_DKDV": "2"},), ("fwd2", (12, 1), FWD2), [("dq3", (12, 1), DQ3), ("dkdv2", (3, 6), DKDV3)]),
    (C257 + ({"MIPIPE_ATTN_BWD_DKDV": "3"},), ("fwd2", (12, 1), FWD2), [("dq3", (12, 1), DQ3), ("dkdv3", (12, 1), DKDV3)]),
    (C257 + (V1,), ("fwd1", (3, 6), 32768), [("dq1", (3, 6), 65536), ("dkdv1", (3, 6), 67584)]),
    # --- short non-causal: key-split forward, one-launch backward; MIPIPE_ATTN_KS2 / BWD_SHORT ---
    (S64 + ({},), ("ks2", (1, 6), 32768), [("short", (2, 6), 50176)]),
    (S64 + ({"MIPIPE_ATTN_KS2": "1"},), ("ks2", (1, 6), 32768), [("short", (2, 6), 50176)]),
    (S64 + ({"MIPIPE_ATTN_KS2": "0"},), ("fwd2", (6, 1), FWD2), [("short", (2, 6), 50176)]),
    (S64 + ({"MIPIPE_ATTN_BWD_SHORT": "1"},), ("ks2", (1, 6), 32768), [("short", (2, 6), 50176)]),
    (S64 + ({"MIPIPE_ATTN_BWD_SHORT": "0"},), ("ks2", (1, 6), 32768), [("dq3", (6, 1), DQ3), ("dkdv3", (6, 1), DKDV3)]),
    (S64 + (V1,), ("fwd1", (1, 6), 32768), [("dq1", (1, 6), 65536), ("dkdv1", (1, 6), 67584)]),
    ((2, 64, 64, 3, 3, 64, True, False, None, {}),             # causal: neither
     ("fwd2", (6, 1), FWD2), [("dq3", (6, 1), DQ3), ("dkdv3", (6, 1), DKDV3)]),
    # key-split: fewer than 256 workgroups of 128 queries
    ((51, 128, 128, 5, 5, 64, False, False, None, {}), ("ks2", (2, 255), 32768), [("short", (4, 255), 50176)]),
    ((64, 128, 128, 4, 4, 64, False, False, None, {}), ("fwd2", (256, 1), FWD2), [("short", (4, 256), 50176)]),
    ((32, 129, 129, 4, 4, 64, False, False, None, {}),         # 2 blocks x 128 = 256
     ("fwd2", (256, 1), FWD2), [("dq3", (256, 1), DQ3), ("dkdv3", (256, 1), DKDV3)]),
    # short: Sq <= 128 and Sk <= 128 and H == Hkv
    ((2, 128, 128, 3, 3, 64, False, False, None, {}), ("ks2", (2, 6), 32768), [("short", (4, 6), 50176)]),
    ((2, 129, 128, 3, 3, 64, False, False, None, {}),
     ("ks2", (3, 6), 32768), [("dq3", (12, 1), DQ3), ("dkdv3", (6, 1), DKDV3)]),
    ((2, 128, 129, 3, 3, 64, False, False, None, {}),          # 3 key tiles: the key-split pairs loop
     ("ks2", (2, 6), 65536), [("dq3", (6, 1), DQ3), ("dkdv3", (12, 1), DKDV3)]),
    ((1, 100, 100, 8, 2, 64, False, False, None, {}),          # GQA leaves short
     ("ks2", (2, 8), 32768), [("dq3", (8, 1), DQ3), ("dkdv3", (2, 1), DKDV3)]),
    # --- head dims: padded to 64 / 128 / 256; v2 / v3 only at 64 ----------------------------------
    (D_ROW(64) + ({},), ("fwd2", (2, 1), FWD2), [("dq3", (2, 1), DQ3), ("dkdv3", (2, 1), DKDV3)]),
    (D_ROW(72) + ({},), ("fwd1", (2, 2), 65536), [("dq1", (2, 2), 131072), ("dkdv1", (2, 2), 133120)]),
    (D_ROW(128) + ({},), ("fwd1", (2, 2), 65536), [("dq1", (2, 2), 131072), ("dkdv1", (2, 2), 133120)]),
    (D_ROW(136) + ({},), ("fwd1", (2, 2), 131072), [("dq1", (2, 2), 131072), ("dkdv1", (2, 2), 132096)]),
    (D_ROW(256) + ({},), ("fwd1", (2, 2), 131072), [("dq1", (2, 2), 131072), ("dkdv1", (2, 2), 132096)]),
    ((2, 100, 100, 3, 3, 128, False, False, None, {}), ("ks2", (2, 6), 65536), [("short", (4, 6), 99328)]),
    ((2, 100, 300, 3, 3, 128, False, False, None, {}),
     ("ks2", (2, 6), 131072), [("dq1", (1, 6), 131072), ("dkdv1", (3, 6), 133120)]),
    ((2, 100, 100, 3, 3, 192, False, False, None, {}),         # d_h 256: no key-split, no short
     ("fwd1", (1, 6), 131072), [("dq1", (1, 6), 131072), ("dkdv1", (1, 6), 132096)]),
    # --- 32-bit buffer offsets: (S + 128) * stride * 2 < 2^31, k / v rows for the forward and dQ,
    #     q / o rows for dK/dV ---------------------------------------------------------------------
    (BIGROW(BIG, BIG, BIG, BIG) + ({},), ("fwd1", (1, 2), 32768), [("dq1", (1, 2), 65536), ("dkdv1", (1, 2), 67584)]),
    (BIGROW(128, BIG, BIG, 128) + ({},), ("fwd1", (1, 2), 32768), [("dq1", (1, 2), 65536), ("dkdv3", (2, 1), DKDV3)]),
    (BIGROW(128, 128, BIG, 128) + ({},), ("fwd1", (1, 2), 32768), [("dq1", (1, 2), 65536), ("dkdv3", (2, 1), DKDV3)]),
    (BIGROW(BIG, 128, 128, BIG) + ({},), ("fwd2", (2, 1), FWD2), [("dq3", (2, 1), DQ3), ("dkdv1", (1, 2), 67584)]),
    (BIGROW(128, 128, 128, BIG) + ({},), ("fwd2", (2, 1), FWD2), [("dq3", (2, 1), DQ3), ("dkdv1", (1, 2), 67584)]),
    (BIGROW(128, 4194296, 4194296, 128) + ({},),               # 256 rows x 2 bytes: 2^31 at stride 2^22
     ("fwd2", (2, 1), FWD2), [("dq3", (2, 1), DQ3), ("dkdv3", (2, 1), DKDV3)]),
    (BIGROW(128, 4194304, 128, 128) + ({},), ("fwd1", (1, 2), 32768), [("dq1", (1, 2), 65536), ("dkdv3", (2, 1), DKDV3)]),
]


@pytest.fixture(scope="module", autouse=True)
def ext():
    e = K.load_ext()
    if e is None or not hasattr(e, "attn_plan"):
        pytest.skip("extension not built")
    return e


def plan(B, Sq, Sk, H, Hkv, D, causal, drop, strides, env):
    qs, ks, vs, os_ = strides or (H * D, Hkv * D, Hkv * D, H * D)
    return ops.attn_plan(B, Sq, Sk, H, Hkv, D, qs, ks, vs, os_, causal, drop, env=env)


def launches(p):
    """every launch of a plan as (kernel, grid, lds)"""
    return [(l["kernel"], tuple(l["grid"]), l["lds"]) for l in [p["fwd"]] + list(p["bwd"])]


def sane(p):
    return all(0 < lds <= LDS_MAX and min(grid) >= 1 for _, grid, lds in launches(p)) and \
        all(l["dp"] in (64, 128, 256) for l in [p["fwd"]] + list(p["bwd"]))


def test_plan_table():
    bad = []
    for args, fwd, bwd in TABLE:
        p = plan(*args)
        if launches(p) != [fwd] + bwd or not sane(p):
            bad.append((args, launches(p), [fwd] + bwd))
    assert not bad, bad


def test_plan_refuses():
    for D, H, Hkv in ((264, 2, 2), (60, 2, 2), (64, 3, 2)):
        with pytest.raises(RuntimeError, match="no kernel"):
            ops.attn_plan(1, 129, 129, H, Hkv, D, H * D, Hkv * D, Hkv * D, H * D, True, False)
    with pytest.raises(RuntimeError, match="MIPIPE_ATTN_NOPE"):
        plan(*C257, {"MIPIPE_ATTN_NOPE": "1"})
    with pytest.raises(RuntimeError, match="not an attention switch"):
        plan(*C257, {"MIPIPE_ATTN": "1"})


def test_plan_default_env_is_process_env():
    if any(k.startswith("MIPIPE_ATTN_") for k in os.environ):
        pytest.skip("an attention switch is set in this process")
    for args, _, _ in TABLE:
        assert plan(*args[:-1], None) == plan(*args[:-1], {}), args


# ------------------------------------------------------------------ against attn_refs.path()
def check_against_path(c, flags):
    """the plan of case ``c`` under the switches ``flags`` (attn_refs.env_flags form) against
    the hand re-statement: the kernels, and what the rest of the label says of grid and LDS"""
    B, Sq, Sk, H, Hkv, D = c.shape()
    path = R.path(c, flags)
    p = ops.attn_plan(B, Sq, Sk, H, Hkv, D, *R.case_strides(c), c.causal, c.p > 0, env=R.plan_env(flags))
    assert R.planned_kernels(p) == R.path_kernels(path), (c.id, path, p)
    assert sane(p), (c.id, p)
    DP = p["fwd"]["dp"]
    assert DP == (64 if D <= 64 else 128 if D <= 128 else 256)
    labels = [path[0]] if path[1].startswith("short") else [path[0]] + path[1].split("+")
    for label, launch in zip(labels, [p["fwd"]] + list(p["bwd"])):
        nheads = B * (Hkv if label.startswith("dkdv") else H)
        m = re.fullmatch(r"(fwd2|dq3|dkdv3)x(\d+)(pair(odd|even))?", label)
        if m:   # x<n>: n pairs (causal) or n blocks of 128 rows, one workgroup each per (b, head)
            n128 = ((Sk if m.group(1) == "dkdv3" else Sq) + 127) // 128
            assert bool(m.group(3)) == c.causal, (c.id, label)
            assert int(m.group(2)) == ((n128 + 1) // 2 if c.causal else n128), (c.id, label)
            assert tuple(launch["grid"]) == (int(m.group(2)) * nheads, 1), (c.id, label, launch)
        elif label.startswith("ks2"):
            assert launch["lds"] == {"ks2-1iter": 4, "ks2-loop": 8}[label] * 64 * DP * 2, (c.id, label, launch)
            assert tuple(launch["grid"]) == ((Sq + 63) // 64, nheads), (c.id, label, launch)
        else:   # the 2-D grids: 128-row blocks x (b, head)
            assert re.fullmatch(r"(fwd1|dq1|dkdv1)dp%d|dq2|dkdv2" % DP, label), (c.id, label)
            n128 = ((Sk if label.startswith("dkdv") else Sq) + 127) // 128
            assert tuple(launch["grid"]) == (n128, nheads), (c.id, label, launch)
    m = re.fullmatch(r"short(\d+)\+(\d+)", path[1])
    if m:
        assert tuple(p["bwd"][0]["grid"]) == (int(m.group(1)) + int(m.group(2)), B * H), (c.id, path, p)


def test_plan_names_what_path_names_default():
    cases = [c for c in R.CASES if c.prec == "bf16"]
    assert len(cases) > 100
    for c in cases:
        check_against_path(c, R.DEFAULT_ENV)
    big = [c for c in cases if c.layout == "bigstride"]
    assert big and all(R.case_strides(c) == (BIG,) * 4 for c in big)


@pytest.mark.parametrize("name", ["v1", "v2"])
def test_plan_names_what_path_names_children(name):
    for c in R.CHILD_CASES:
        check_against_path(c, R.env_flags(R.CHILD_ENVS[name]))
