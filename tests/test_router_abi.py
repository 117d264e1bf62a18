"""C ABI of the router entry points (include/fql_int4.h, csrc/fql_router.h): declared, exported, and the return codes
that are decided before any HIP call.

The table is written out in the style of tests/test_dispatch_contract.py: (entry point, arguments, expected code), the
codes read off the documented order -- element type, then shape, then the empty call, then pointers.  Every pointer is
NULL: no row hands the library memory a kernel could touch if a refusal were lost."""
import ctypes

import pytest

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

ROUTER = ("fql_router_topk_fwd", "fql_router_topk_bwd")
OK, NULLP, SHAPE, DTYPE = 0, -1, -2, -8
F32, F16, BF16, BADT = 0, 1, 2, 3
N_ = None                      # a NULL pointer


@pytest.fixture(scope="module")
def lib():
    from fused_int4_amd import _native
    return _native.lib()


def test_declared_and_exported(lib):
    import test_c_abi
    names = test_c_abi.declared_symbols()
    raw = ctypes.CDLL(lib._name)
    for name in ROUTER:
        assert name in names, name
        assert hasattr(raw, name), name
    assert lib.fql_version() >= 270


ROWS = [
    # ---- fql_router_topk_fwd(logits, logits_dtype, T, E, top_k, renormalize, indices, weights, probs, stream)
    ("fql_router_topk_fwd", (N_, BADT, 4, 8, 2, 1, N_, N_, N_, N_), DTYPE),
    ("fql_router_topk_fwd", (N_, -1, -4, 0, 0, 1, N_, N_, N_, N_), DTYPE),               # the element type before the shape
    ("fql_router_topk_fwd", (N_, BADT, 0, 8, 2, 1, N_, N_, N_, N_), DTYPE),              # ... and before the empty call
    ("fql_router_topk_fwd", (N_, F32, -1, 8, 2, 1, N_, N_, N_, N_), SHAPE),
    ("fql_router_topk_fwd", (N_, F32, 4, 0, 1, 1, N_, N_, N_, N_), SHAPE),
    ("fql_router_topk_fwd", (N_, F16, 4, 129, 2, 1, N_, N_, N_, N_), SHAPE),
    ("fql_router_topk_fwd", (N_, BF16, 4, 8, 0, 0, N_, N_, N_, N_), SHAPE),
    ("fql_router_topk_fwd", (N_, F32, 4, 3, 4, 1, N_, N_, N_, N_), SHAPE),               # top_k > E
    ("fql_router_topk_fwd", (N_, F32, 4, 64, 9, 1, N_, N_, N_, N_), SHAPE),              # top_k > 8
    ("fql_router_topk_fwd", (N_, F32, 0, 129, 2, 1, N_, N_, N_, N_), SHAPE),             # the shape before the empty call
    ("fql_router_topk_fwd", (N_, F32, 0, 8, 2, 1, N_, N_, N_, N_), OK),
    ("fql_router_topk_fwd", (N_, BF16, 0, 128, 8, 0, N_, N_, N_, N_), OK),
    ("fql_router_topk_fwd", (N_, F32, 4, 8, 2, 1, N_, N_, N_, N_), NULLP),
    ("fql_router_topk_fwd", (N_, F16, 1, 1, 1, 0, N_, N_, N_, N_), NULLP),
    ("fql_router_topk_fwd", (N_, BF16, 257, 128, 8, 1, N_, N_, N_, N_), NULLP),
    # ---- fql_router_topk_bwd(logits, logits_dtype, indices, grad_weights, grad_probs, grad_logits, T, E, top_k, renormalize, stream)
    ("fql_router_topk_bwd", (N_, BADT, N_, N_, N_, N_, 4, 8, 2, 1, N_), DTYPE),
    ("fql_router_topk_bwd", (N_, 7, N_, N_, N_, N_, -1, 200, 0, 1, N_), DTYPE),
    ("fql_router_topk_bwd", (N_, BADT, N_, N_, N_, N_, 0, 8, 2, 1, N_), DTYPE),
    ("fql_router_topk_bwd", (N_, F32, N_, N_, N_, N_, -1, 8, 2, 1, N_), SHAPE),
    ("fql_router_topk_bwd", (N_, F32, N_, N_, N_, N_, 4, 0, 1, 1, N_), SHAPE),
    ("fql_router_topk_bwd", (N_, F16, N_, N_, N_, N_, 4, 129, 2, 0, N_), SHAPE),
    ("fql_router_topk_bwd", (N_, BF16, N_, N_, N_, N_, 4, 8, 0, 1, N_), SHAPE),
    ("fql_router_topk_bwd", (N_, F32, N_, N_, N_, N_, 4, 3, 4, 1, N_), SHAPE),
    ("fql_router_topk_bwd", (N_, F32, N_, N_, N_, N_, 4, 64, 9, 0, N_), SHAPE),
    ("fql_router_topk_bwd", (N_, F32, N_, N_, N_, N_, 0, 8, 9, 1, N_), SHAPE),
    ("fql_router_topk_bwd", (N_, F32, N_, N_, N_, N_, 0, 8, 2, 1, N_), OK),
    ("fql_router_topk_bwd", (N_, F16, N_, N_, N_, N_, 0, 1, 1, 0, N_), OK),
    ("fql_router_topk_bwd", (N_, F32, N_, N_, N_, N_, 4, 8, 2, 1, N_), NULLP),
    ("fql_router_topk_bwd", (N_, BF16, N_, N_, N_, N_, 257, 128, 8, 0, N_), NULLP),
]


@pytest.mark.parametrize("row", range(len(ROWS)), ids=lambda i: f"{i}-{ROWS[i][0]}")
def test_return_code(lib, row):
    name, args, expected = ROWS[row]
    assert getattr(lib, name)(*args) == expected, (name, args)
