"""C ABI of the typed combine (include/fql_int4.h, csrc/fql_routing.h): fql_combine and fql_combine_bwd are declared and
exported, and their return codes come in the order the header freezes -- shape, element type, the empty call, pointers,
the token limit (forward), alignment -- all decided before the first HIP call.

The table is written out in the style of tests/test_router_abi.py.  Every row up to the pointer checks passes NULL for
every pointer.  The rows behind them (the token limit, alignment) need non-NULL pointers to get that far: they pass small
integers that are no allocation's address, and every one of them ends in a refusal, so nothing is launched."""
import ctypes

import pytest

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

COMBINE = ("fql_combine", "fql_combine_bwd")
OK, NULLP, SHAPE, ALIGNMENT, DTYPE = 0, -1, -2, -7, -8
F32, F16, BF16, BADT = 0, 1, 2, 3
N_ = None                      # a NULL pointer
A = 0x1000                     # "aligned" stand-ins for pointers of refused calls (never dereferenced)
A2, A1 = A + 2, A + 1          # aligned to 2 bytes only / to nothing


@pytest.fixture(scope="module")
def lib():
    from fused_int4_amd import _native
    return _native.lib()


def test_declared_and_exported(lib):
    import test_c_abi
    names = test_c_abi.declared_symbols()
    raw = ctypes.CDLL(lib._name)
    for name in COMBINE:
        assert name in names, name
        assert hasattr(raw, name), name
    assert lib.fql_version() >= 290


ROWS = [
    # ---- fql_combine(y, in_dtype, pos_of_slot, weights, addend, addend_weight, out, out_dtype, T, top_k, N, R, stream)
    ("fql_combine", (N_, F32, N_, N_, N_, N_, N_, F32, -1, 2, 8, 8, N_), SHAPE),
    ("fql_combine", (N_, BF16, N_, N_, N_, N_, N_, BF16, 4, 0, 8, 8, N_), SHAPE),
    ("fql_combine", (N_, F16, N_, N_, N_, N_, N_, F32, 4, 2, -8, 8, N_), SHAPE),
    ("fql_combine", (N_, F32, N_, N_, N_, N_, N_, F16, 4, 2, 8, -1, N_), SHAPE),
    ("fql_combine", (N_, BADT, N_, N_, N_, N_, N_, BADT, 4, -2, 8, 8, N_), SHAPE),          # the shape before the element type
    ("fql_combine", (N_, F32, N_, N_, N_, N_, N_, F32, 0, 0, 8, 8, N_), SHAPE),              # ... and before the empty call
    ("fql_combine", (N_, BADT, N_, N_, N_, N_, N_, F32, 4, 2, 8, 8, N_), DTYPE),
    ("fql_combine", (N_, BF16, N_, N_, N_, N_, N_, -1, 4, 2, 8, 8, N_), DTYPE),
    ("fql_combine", (N_, F32, N_, N_, N_, N_, N_, BADT, 0, 2, 8, 8, N_), DTYPE),             # the element type before the empty call
    ("fql_combine", (N_, BADT, N_, N_, N_, N_, N_, BF16, 4, 2, 0, 8, N_), DTYPE),
    ("fql_combine", (N_, F32, N_, N_, N_, N_, N_, F32, 0, 2, 8, 8, N_), OK),
    ("fql_combine", (N_, BF16, N_, N_, N_, N_, N_, BF16, 4, 2, 0, 8, N_), OK),
    ("fql_combine", (N_, F16, N_, N_, N_, N_, N_, F32, 0, 8, 0, 0, N_), OK),
    ("fql_combine", (N_, BF16, N_, N_, N_, N_, N_, F32, 70000, 2, 0, 8, N_), OK),            # the empty call before the token limit
    ("fql_combine", (N_, F32, N_, N_, N_, N_, N_, F32, 4, 2, 8, 8, N_), NULLP),
    ("fql_combine", (N_, BF16, N_, N_, N_, N_, N_, BF16, 4, 2, 8, 8, N_), NULLP),
    ("fql_combine", (A, BF16, A, N_, N_, N_, N_, BF16, 4, 2, 8, 8, N_), NULLP),              # out
    ("fql_combine", (A, BF16, N_, N_, N_, N_, A, BF16, 4, 2, 8, 8, N_), NULLP),              # pos_of_slot
    ("fql_combine", (A, BF16, A, N_, N_, N_, A, BF16, 4, 2, 8, 0, N_), NULLP),               # R == 0: no row to point at
    ("fql_combine", (A, BF16, A, A, N_, A, A, BF16, 4, 2, 8, 8, N_), NULLP),                 # addend_weight without addend
    ("fql_combine", (N_, F16, N_, N_, N_, N_, N_, F16, 70000, 2, 8, 8, N_), NULLP),          # pointers before the token limit
    ("fql_combine", (A, F32, A, A, N_, N_, A, F32, 65536, 2, 8, 8, N_), SHAPE),
    ("fql_combine", (A1, BF16, A, A, A, A, A, BF16, 65536, 2, 8, 8, N_), SHAPE),             # the token limit before alignment
    ("fql_combine", (A1, BF16, A, A, N_, N_, A, BF16, 4, 2, 8, 8, N_), ALIGNMENT),           # y
    ("fql_combine", (A2, F32, A, A, N_, N_, A, F32, 4, 2, 8, 8, N_), ALIGNMENT),             # (float32 alone: not the _f32 twin's order)
    ("fql_combine", (A, F16, A, A, A1, N_, A, F16, 4, 2, 8, 8, N_), ALIGNMENT),              # addend
    ("fql_combine", (A, BF16, A, A, A, A, A2, F32, 4, 2, 8, 8, N_), ALIGNMENT),              # out, float32
    ("fql_combine", (A, F32, A, A, N_, N_, A1, F16, 4, 2, 8, 8, N_), ALIGNMENT),             # out, 16-bit
    ("fql_combine", (A, BF16, A2, A, N_, N_, A, BF16, 4, 2, 8, 8, N_), ALIGNMENT),           # pos_of_slot
    ("fql_combine", (A, BF16, A, A2, N_, N_, A, BF16, 4, 2, 8, 8, N_), ALIGNMENT),           # weights
    ("fql_combine", (A, BF16, A, A, A, A2, A, BF16, 4, 2, 8, 8, N_), ALIGNMENT),             # addend_weight
    # ---- fql_combine_bwd(grad_out, out_dtype, y, pos_of_slot, weights, addend, addend_weight, in_dtype,
    #                      grad_y, grad_weights, grad_addend, grad_addend_weight, T, top_k, N, rows, stream)
    ("fql_combine_bwd", (N_, F32, N_, N_, N_, N_, N_, F32, N_, N_, N_, N_, -1, 2, 8, 8, N_), SHAPE),
    ("fql_combine_bwd", (N_, BF16, N_, N_, N_, N_, N_, BF16, N_, N_, N_, N_, 4, 0, 8, 8, N_), SHAPE),
    ("fql_combine_bwd", (N_, F16, N_, N_, N_, N_, N_, F32, N_, N_, N_, N_, 4, 2, -1, 8, N_), SHAPE),
    ("fql_combine_bwd", (N_, F32, N_, N_, N_, N_, N_, F16, N_, N_, N_, N_, 4, 2, 8, -8, N_), SHAPE),
    ("fql_combine_bwd", (N_, F32, N_, N_, N_, N_, N_, F32, N_, N_, N_, N_, 4, 2, 8, 0, N_), SHAPE),     # slots with no rows
    ("fql_combine_bwd", (N_, BADT, N_, N_, N_, N_, N_, BADT, N_, N_, N_, N_, 4, 2, 8, 0, N_), SHAPE),   # before the element type
    ("fql_combine_bwd", (N_, BADT, N_, N_, N_, N_, N_, F32, N_, N_, N_, N_, 4, 2, 8, 8, N_), DTYPE),
    ("fql_combine_bwd", (N_, BF16, N_, N_, N_, N_, N_, 7, N_, N_, N_, N_, 4, 2, 8, 8, N_), DTYPE),
    ("fql_combine_bwd", (N_, BADT, N_, N_, N_, N_, N_, F32, N_, N_, N_, N_, 0, 2, 8, 8, N_), DTYPE),    # before the empty call
    ("fql_combine_bwd", (N_, F32, N_, N_, N_, N_, N_, F32, N_, N_, N_, N_, 0, 2, 8, 8, N_), OK),
    ("fql_combine_bwd", (N_, BF16, N_, N_, N_, N_, N_, BF16, N_, N_, N_, N_, 0, 2, 8, 0, N_), OK),      # T == 0 needs no rows
    ("fql_combine_bwd", (N_, F16, N_, N_, N_, N_, N_, F16, N_, N_, N_, N_, 4, 2, 0, 8, N_), OK),        # N == 0, no dot product wanted
    ("fql_combine_bwd", (N_, F32, N_, N_, N_, N_, N_, F32, N_, N_, N_, N_, 4, 2, 8, 8, N_), NULLP),
    ("fql_combine_bwd", (N_, BF16, N_, N_, N_, N_, N_, BF16, N_, N_, N_, N_, 4, 2, 8, 8, N_), NULLP),
    ("fql_combine_bwd", (N_, BF16, N_, N_, N_, N_, N_, BF16, N_, A, N_, N_, 4, 2, 0, 8, N_), NULLP),    # N == 0 with grad_weights: pos_of_slot
    ("fql_combine_bwd", (N_, BF16, A, A, N_, N_, N_, BF16, A, N_, N_, N_, 4, 2, 8, 8, N_), NULLP),      # grad_out
    ("fql_combine_bwd", (A, BF16, A, A, N_, N_, N_, BF16, N_, N_, N_, N_, 4, 2, 8, 8, N_), NULLP),      # grad_y
    ("fql_combine_bwd", (A, BF16, N_, A, A, N_, N_, BF16, A, A, N_, N_, 4, 2, 8, 8, N_), NULLP),        # y for grad_weights
    ("fql_combine_bwd", (A, BF16, A, A, A, N_, A, BF16, A, A, N_, N_, 4, 2, 8, 8, N_), NULLP),          # addend_weight without addend
    ("fql_combine_bwd", (A, BF16, A, A, A, N_, N_, BF16, A, A, N_, A, 4, 2, 8, 8, N_), NULLP),          # grad_addend_weight without addend
    ("fql_combine_bwd", (A1, BF16, A, A, A, N_, N_, BF16, A, A, N_, N_, 4, 2, 8, 8, N_), ALIGNMENT),    # grad_out
    ("fql_combine_bwd", (A2, F32, A, A, A, N_, N_, F32, A, A, N_, N_, 4, 2, 8, 8, N_), ALIGNMENT),      # (float32 alone as well)
    ("fql_combine_bwd", (A, BF16, A1, A, A, N_, N_, F16, A, A, N_, N_, 4, 2, 8, 8, N_), ALIGNMENT),     # y
    ("fql_combine_bwd", (A, F32, A, A, A, N_, N_, F32, A2, A, N_, N_, 4, 2, 8, 8, N_), ALIGNMENT),      # grad_y
    ("fql_combine_bwd", (A, BF16, A, A, A, A, A, BF16, A, A, A1, A, 4, 2, 8, 8, N_), ALIGNMENT),        # grad_addend
    ("fql_combine_bwd", (A, BF16, A, A, A, A, A, BF16, A, A, A, A2, 4, 2, 8, 8, N_), ALIGNMENT),        # grad_addend_weight
    ("fql_combine_bwd", (A, BF16, A, A, A, A, A, BF16, A, A2, A, A, 4, 2, 8, 8, N_), ALIGNMENT),        # grad_weights
]


@pytest.mark.parametrize("row", range(len(ROWS)), ids=lambda i: f"{i}-{ROWS[i][0]}")
def test_return_code(lib, row):
    name, args, expected = ROWS[row]
    assert getattr(lib, name)(*args) == expected, (name, args)
