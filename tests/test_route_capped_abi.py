"""C ABI of the capped plan and the sparse combine pair (include/fql_int4.h, FQL_VERSION 320): fql_route_plan_capped_i32,
fql_combine_sparse and fql_combine_sparse_bwd are declared and exported, the header still compiles as C, and their return
codes come in the order the header freezes, all decided before the first HIP call.

The table is written out in the style of tests/test_combine_abi.py: every row up to the pointer checks passes NULL for
every pointer; the rows behind them pass small integers that are no allocation's address, and every one of them ends in a
refusal (or in the empty call), so nothing is launched."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT

NAMES = ("fql_route_plan_capped_i32", "fql_combine_sparse", "fql_combine_sparse_bwd")
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
    from fused_int4_amd import _native
    names = test_c_abi.declared_symbols()
    raw = ctypes.CDLL(lib._name)
    for name in NAMES:
        assert name in names, name
        assert hasattr(raw, name), name
        assert name in _native.exported_symbols(), name
    assert lib.fql_version() >= 320


def test_header_compiles_as_plain_c_and_declares_the_three():
    src = ("#include \"fql_int4.h\"\n"
           "int main(void){\n"
           "  int (*p)(const int32_t *, int, int, int, const uint8_t *, int, int32_t *, int32_t *, int32_t *, int32_t *,\n"
           "           int32_t *, void *) = fql_route_plan_capped_i32;\n"
           "  int (*f)(const void *, int, const int32_t *, const float *, const void *, const float *, void *, int, int, int,\n"
           "           int, int, void *) = fql_combine_sparse;\n"
           "  int (*b)(const void *, int, const void *, const int32_t *, const float *, const void *, const float *, int,\n"
           "           void *, float *, void *, float *, int, int, int, int, void *) = fql_combine_sparse_bwd;\n"
           "  return (p != 0 && f != 0 && b != 0 && FQL_VERSION >= 320) ? 0 : 1;}\n")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                          "-x", "c", "-"], input=src.encode(), capture_output=True)
    assert out.returncode == 0, out.stderr.decode()


PLAN = "fql_route_plan_capped_i32"
FWD, BWD = "fql_combine_sparse", "fql_combine_sparse_bwd"
ROWS = [
    # ---- fql_route_plan_capped_i32(expert_of_slot, n_slots, top_k, E, token_mask, capacity, demand, counts, offsets,
    #                                token_of_sorted, pos_of_slot, stream)
    (PLAN, (N_, -1, 2, 8, N_, 0, N_, N_, N_, N_, N_, N_), SHAPE),               # n_slots < 0
    (PLAN, (N_, 8, 0, 8, N_, 0, N_, N_, N_, N_, N_, N_), SHAPE),                # top_k <= 0
    (PLAN, (N_, 8, -2, 8, N_, 0, N_, N_, N_, N_, N_, N_), SHAPE),
    (PLAN, (N_, 8, 2, 0, N_, 0, N_, N_, N_, N_, N_, N_), SHAPE),                # E outside [1, 128]
    (PLAN, (N_, 8, 2, 129, N_, 0, N_, N_, N_, N_, N_, N_), SHAPE),
    (PLAN, (N_, 8, 2, 8, N_, -1, N_, N_, N_, N_, N_, N_), SHAPE),               # capacity < 0
    (PLAN, (N_, 9, 2, 8, N_, 0, N_, N_, N_, N_, N_, N_), SHAPE),                # n_slots % top_k != 0
    (PLAN, (A, 9, 2, 8, A, 4, A, A, A, A, A, N_), SHAPE),                       # ... with every pointer given
    (PLAN, (A, 8, 2, 8, A, -3, A, A, A, A, A, N_), SHAPE),
    (PLAN, (N_, 8, 2, 8, N_, 0, N_, N_, N_, N_, N_, N_), NULLP),                # the shape before the pointers
    (PLAN, (N_, 0, 2, 8, N_, 0, N_, N_, N_, N_, N_, N_), NULLP),                # n_slots == 0 still writes three tables
    (PLAN, (A, 8, 2, 128, N_, 3, N_, A, A, A, A, N_), NULLP),                   # demand
    (PLAN, (A, 8, 2, 128, N_, 3, A, N_, A, A, A, N_), NULLP),                   # counts
    (PLAN, (A, 8, 2, 128, N_, 3, A, A, N_, A, A, N_), NULLP),                   # offsets
    (PLAN, (N_, 8, 2, 1, N_, 0, A, A, A, A, A, N_), NULLP),                     # expert_of_slot
    (PLAN, (A, 8, 2, 1, A, 0, A, A, A, N_, A, N_), NULLP),                      # token_of_sorted
    (PLAN, (A, 8, 2, 1, A, 0, A, A, A, A, N_, N_), NULLP),                      # pos_of_slot
    # ---- fql_combine_sparse(y, in_dtype, pos_of_slot, weights, addend, addend_weight, out, out_dtype, T, top_k, N, R,
    #                         stream): fql_combine's codes and order
    (FWD, (N_, F32, N_, N_, N_, N_, N_, F32, -1, 2, 8, 8, N_), SHAPE),
    (FWD, (N_, BF16, N_, N_, N_, N_, N_, BF16, 4, 0, 8, 8, N_), SHAPE),
    (FWD, (N_, F16, N_, N_, N_, N_, N_, F32, 4, 2, -8, 8, N_), SHAPE),
    (FWD, (N_, F32, N_, N_, N_, N_, N_, F16, 4, 2, 8, -1, N_), SHAPE),
    (FWD, (N_, BADT, N_, N_, N_, N_, N_, BADT, 4, -2, 8, 8, N_), SHAPE),          # the shape before the element type
    (FWD, (N_, F32, N_, N_, N_, N_, N_, F32, 0, 0, 8, 8, N_), SHAPE),              # ... and before the empty call
    (FWD, (N_, BADT, N_, N_, N_, N_, N_, F32, 4, 2, 8, 8, N_), DTYPE),
    (FWD, (N_, BF16, N_, N_, N_, N_, N_, -1, 4, 2, 8, 8, N_), DTYPE),
    (FWD, (N_, F32, N_, N_, N_, N_, N_, BADT, 0, 2, 8, 8, N_), DTYPE),             # the element type before the empty call
    (FWD, (N_, F32, N_, N_, N_, N_, N_, F32, 0, 2, 8, 8, N_), OK),
    (FWD, (N_, BF16, N_, N_, N_, N_, N_, BF16, 4, 2, 0, 8, N_), OK),
    (FWD, (N_, BF16, N_, N_, N_, N_, N_, F32, 70000, 2, 0, 8, N_), OK),            # the empty call before the token limit
    (FWD, (N_, F32, N_, N_, N_, N_, N_, F32, 4, 2, 8, 8, N_), NULLP),
    (FWD, (A, BF16, A, N_, N_, N_, N_, BF16, 4, 2, 8, 8, N_), NULLP),              # out
    (FWD, (A, BF16, N_, N_, N_, N_, A, BF16, 4, 2, 8, 8, N_), NULLP),              # pos_of_slot
    (FWD, (A, BF16, A, N_, N_, N_, A, BF16, 4, 2, 8, 0, N_), NULLP),               # R == 0: no row to point at
    (FWD, (A, BF16, A, A, N_, A, A, BF16, 4, 2, 8, 8, N_), NULLP),                 # addend_weight without addend
    (FWD, (N_, F16, N_, N_, N_, N_, N_, F16, 70000, 2, 8, 8, N_), NULLP),          # pointers before the token limit
    (FWD, (A, F32, A, A, N_, N_, A, F32, 65536, 2, 8, 8, N_), SHAPE),
    (FWD, (A1, BF16, A, A, A, A, A, BF16, 65536, 2, 8, 8, N_), SHAPE),             # the token limit before alignment
    (FWD, (A1, BF16, A, A, N_, N_, A, BF16, 4, 2, 8, 8, N_), ALIGNMENT),           # y
    (FWD, (A, F16, A, A, A1, N_, A, F16, 4, 2, 8, 8, N_), ALIGNMENT),              # addend
    (FWD, (A, BF16, A, A, A, A, A2, F32, 4, 2, 8, 8, N_), ALIGNMENT),              # out
    (FWD, (A, BF16, A2, A, N_, N_, A, BF16, 4, 2, 8, 8, N_), ALIGNMENT),           # pos_of_slot
    (FWD, (A, BF16, A, A2, N_, N_, A, BF16, 4, 2, 8, 8, N_), ALIGNMENT),           # weights
    (FWD, (A, BF16, A, A, A, A2, A, BF16, 4, 2, 8, 8, N_), ALIGNMENT),             # addend_weight
    # ---- fql_combine_sparse_bwd(grad_out, out_dtype, y, pos_of_slot, weights, addend, addend_weight, in_dtype, grad_y,
    #                             grad_weights, grad_addend, grad_addend_weight, T, top_k, N, rows, stream)
    (BWD, (N_, F32, N_, N_, N_, N_, N_, F32, N_, N_, N_, N_, -1, 2, 8, 8, N_), SHAPE),
    (BWD, (N_, BF16, N_, N_, N_, N_, N_, BF16, N_, N_, N_, N_, 4, 0, 8, 8, N_), SHAPE),
    (BWD, (N_, F16, N_, N_, N_, N_, N_, F32, N_, N_, N_, N_, 4, 2, -1, 8, N_), SHAPE),
    (BWD, (N_, F32, N_, N_, N_, N_, N_, F16, N_, N_, N_, N_, 4, 2, 8, -8, N_), SHAPE),
    (BWD, (N_, F32, N_, N_, N_, N_, N_, F32, N_, N_, N_, N_, 4, 2, 8, 0, N_), SHAPE),     # slots with no rows
    (BWD, (N_, BADT, N_, N_, N_, N_, N_, BADT, N_, N_, N_, N_, 4, 2, 8, 0, N_), SHAPE),   # before the element type
    (BWD, (N_, BADT, N_, N_, N_, N_, N_, F32, N_, N_, N_, N_, 4, 2, 8, 8, N_), DTYPE),
    (BWD, (N_, BF16, N_, N_, N_, N_, N_, 7, N_, N_, N_, N_, 4, 2, 8, 8, N_), DTYPE),
    (BWD, (N_, BADT, N_, N_, N_, N_, N_, F32, N_, N_, N_, N_, 0, 2, 8, 8, N_), DTYPE),    # before the empty call
    (BWD, (N_, F32, N_, N_, N_, N_, N_, F32, N_, N_, N_, N_, 0, 2, 8, 8, N_), OK),
    (BWD, (N_, BF16, N_, N_, N_, N_, N_, BF16, N_, N_, N_, N_, 0, 2, 8, 0, N_), OK),      # T == 0 needs no rows
    (BWD, (N_, F16, N_, N_, N_, N_, N_, F16, N_, N_, N_, N_, 4, 2, 0, 8, N_), OK),        # N == 0, no dot product wanted
    (BWD, (N_, F32, N_, N_, N_, N_, N_, F32, N_, N_, N_, N_, 4, 2, 8, 8, N_), NULLP),
    (BWD, (N_, BF16, N_, N_, N_, N_, N_, BF16, N_, A, N_, N_, 4, 2, 0, 8, N_), NULLP),    # N == 0 with grad_weights: pos_of_slot
    (BWD, (N_, BF16, A, A, N_, N_, N_, BF16, A, N_, N_, N_, 4, 2, 8, 8, N_), NULLP),      # grad_out
    (BWD, (A, BF16, A, A, N_, N_, N_, BF16, N_, N_, N_, N_, 4, 2, 8, 8, N_), NULLP),      # grad_y
    (BWD, (A, BF16, N_, A, A, N_, N_, BF16, A, A, N_, N_, 4, 2, 8, 8, N_), NULLP),        # y for grad_weights
    (BWD, (A, BF16, A, A, A, N_, A, BF16, A, A, N_, N_, 4, 2, 8, 8, N_), NULLP),          # addend_weight without addend
    (BWD, (A, BF16, A, A, A, N_, N_, BF16, A, A, N_, A, 4, 2, 8, 8, N_), NULLP),          # grad_addend_weight without addend
    (BWD, (A1, BF16, A, A, A, N_, N_, BF16, A, A, N_, N_, 4, 2, 8, 8, N_), ALIGNMENT),    # grad_out
    (BWD, (A, BF16, A1, A, A, N_, N_, F16, A, A, N_, N_, 4, 2, 8, 8, N_), ALIGNMENT),     # y
    (BWD, (A, F32, A, A, A, N_, N_, F32, A2, A, N_, N_, 4, 2, 8, 8, N_), ALIGNMENT),      # grad_y
    (BWD, (A, BF16, A, A, A, A, A, BF16, A, A, A1, A, 4, 2, 8, 8, N_), ALIGNMENT),        # grad_addend
    (BWD, (A, BF16, A, A, A, A, A, BF16, A, A, A, A2, 4, 2, 8, 8, N_), ALIGNMENT),        # grad_addend_weight
    (BWD, (A, BF16, A, A, A, A, A, BF16, A, A2, A, A, 4, 2, 8, 8, N_), ALIGNMENT),        # grad_weights
]


@pytest.mark.parametrize("row", range(len(ROWS)), ids=lambda i: f"{i}-{ROWS[i][0]}")
def test_return_code(lib, row):
    name, args, expected = ROWS[row]
    assert getattr(lib, name)(*args) == expected, (name, args)


def test_the_sparse_pair_answers_as_the_dense_pair_does(lib):
    """Every refused or empty call of the table gets the same code from fql_combine / fql_combine_bwd."""
    for name, args, expected in ROWS:
        if name != PLAN:
            assert getattr(lib, name.replace("_sparse", ""))(*args) == expected, (name, args)
