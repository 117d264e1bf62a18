"""C ABI of the scored router (include/fql_int4.h, csrc/fql_router_score.h): declared, exported, the header compiles as
C, and the return codes that are decided before any HIP call.

The table is that of tests/test_router_abi.py: (entry point, arguments, expected code), the codes read off the documented
order -- element type, then shape, then the empty call, then pointers.  Every pointer is NULL: no row hands the library
memory a kernel could touch if a refusal were lost."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT

SCORE = ("fql_router_score_topk_fwd", "fql_router_score_topk_bwd")
OK, NULLP, SHAPE, DTYPE = 0, -1, -2, -8
F32, F16, BF16, BADT = 0, 1, 2, 3
N_ = None                      # a NULL pointer
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def lib():
    from fused_int4_amd import _native
    return _native.lib()


def test_declared_and_exported(lib):
    import test_c_abi
    names = test_c_abi.declared_symbols()
    raw = ctypes.CDLL(lib._name)
    for name in SCORE:
        assert name in names, name
        assert hasattr(raw, name), name
    assert lib.fql_version() >= 280


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "fql_int4.h"\n'
                   "int use(void) { return fql_router_score_topk_fwd(0, 0, 0, 8, 2, 1, 0, 4, 2, 2, 1, 2.5f, 0, 0, 0, 0)\n"
                   "                     + fql_router_score_topk_bwd(0, 0, 0, 0, 0, 0, 0, 8, 2, 1, 1, 2.5f, 0); }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", str(tmp_path / "use.o")])


def fwd(dtype=F32, T=4, E=8, top_k=2, scoring=1, n_group=4, topk_group=2, group_top=2, renormalize=1, scale=2.5):
    """fql_router_score_topk_fwd(logits, logits_dtype, T, E, top_k, scoring, select_bias, n_group, topk_group, group_top,
    renormalize, scale, indices, weights, scores, stream), every pointer NULL."""
    return ("fql_router_score_topk_fwd",
            (N_, dtype, T, E, top_k, scoring, N_, n_group, topk_group, group_top, renormalize, scale, N_, N_, N_, N_))


def bwd(dtype=F32, T=4, E=8, top_k=2, scoring=1, renormalize=1, scale=2.5):
    """fql_router_score_topk_bwd(logits, logits_dtype, indices, grad_weights, grad_scores, grad_logits, T, E, top_k,
    scoring, renormalize, scale, stream), every pointer NULL."""
    return ("fql_router_score_topk_bwd", (N_, dtype, N_, N_, N_, N_, T, E, top_k, scoring, renormalize, scale, N_))


ROWS = [
    # ---- the forward
    (fwd(dtype=BADT), DTYPE),
    (fwd(dtype=-1, T=-4, E=0, top_k=0, scoring=7, n_group=0, scale=NAN), DTYPE),          # the element type before the shape
    (fwd(dtype=BADT, T=0), DTYPE),                                                        # ... and before the empty call
    (fwd(T=-1), SHAPE),
    (fwd(E=0, top_k=1, n_group=1, topk_group=1), SHAPE),
    (fwd(dtype=F16, E=129, n_group=1, topk_group=1), SHAPE),
    (fwd(dtype=BF16, top_k=0), SHAPE),
    (fwd(E=3, top_k=4, n_group=1, topk_group=1), SHAPE),                                  # top_k > E
    (fwd(E=64, top_k=9, n_group=1, topk_group=1), SHAPE),                                 # top_k > 8
    (fwd(scoring=2), SHAPE),
    (fwd(scoring=-1), SHAPE),
    (fwd(n_group=0, topk_group=1), SHAPE),
    (fwd(E=64, n_group=16, topk_group=16), SHAPE),                                        # n_group > 8
    (fwd(E=60, n_group=8, topk_group=8), SHAPE),                                          # E % n_group != 0
    (fwd(topk_group=0), SHAPE),
    (fwd(topk_group=5), SHAPE),                                                           # topk_group > n_group
    (fwd(E=8, top_k=4, n_group=4, topk_group=1), SHAPE),                                  # the chosen groups hold 2 < top_k
    (fwd(group_top=0), SHAPE),
    (fwd(group_top=3), SHAPE),
    (fwd(scale=INF), SHAPE),
    (fwd(scale=-INF), SHAPE),
    (fwd(scale=NAN), SHAPE),
    (fwd(T=0, E=129, n_group=1, topk_group=1), SHAPE),                                    # the shape before the empty call
    (fwd(T=0, scoring=2), SHAPE),
    (fwd(T=0, topk_group=5), SHAPE),
    (fwd(T=0, scale=NAN), SHAPE),
    (fwd(T=0), OK),
    (fwd(dtype=BF16, T=0, E=128, top_k=8, scoring=0, n_group=8, topk_group=4, group_top=1, renormalize=0, scale=1.0), OK),
    (fwd(T=0, E=1, top_k=1, n_group=1, topk_group=1), OK),
    (fwd(), NULLP),
    (fwd(dtype=F16, T=1, E=1, top_k=1, scoring=0, n_group=1, topk_group=1, group_top=1, renormalize=0, scale=0.0), NULLP),
    (fwd(dtype=BF16, T=257, E=128, top_k=8, n_group=8, topk_group=4), NULLP),
    (fwd(E=60, top_k=8, n_group=4, topk_group=2, scale=-1.0), NULLP),                     # a negative scale is a scale
    # ---- the backward (no groups: the indices are saved)
    (bwd(dtype=BADT), DTYPE),
    (bwd(dtype=7, T=-1, E=200, top_k=0, scoring=5, scale=INF), DTYPE),
    (bwd(dtype=BADT, T=0), DTYPE),
    (bwd(T=-1), SHAPE),
    (bwd(E=0, top_k=1), SHAPE),
    (bwd(dtype=F16, E=129), SHAPE),
    (bwd(dtype=BF16, top_k=0), SHAPE),
    (bwd(E=3, top_k=4), SHAPE),
    (bwd(E=64, top_k=9), SHAPE),
    (bwd(scoring=2), SHAPE),
    (bwd(scoring=-1), SHAPE),
    (bwd(scale=INF), SHAPE),
    (bwd(scale=NAN), SHAPE),
    (bwd(T=0, top_k=9), SHAPE),
    (bwd(T=0, scoring=2), SHAPE),
    (bwd(T=0), OK),
    (bwd(dtype=F16, T=0, E=1, top_k=1, scoring=0, renormalize=0, scale=1.0), OK),
    (bwd(), NULLP),
    (bwd(dtype=BF16, T=257, E=128, top_k=8, scoring=0, renormalize=0), NULLP),
]


@pytest.mark.parametrize("row", range(len(ROWS)), ids=lambda i: f"{i}-{ROWS[i][0][0]}")
def test_return_code(lib, row):
    (name, args), expected = ROWS[row]
    assert getattr(lib, name)(*args) == expected, (name, args)
