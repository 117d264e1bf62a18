"""The split-K policy of the three dense 4-bit float families (MXFP4, NVFP4, the NF4 code book) without a GPU, through
their fql_tune_*_linear_kernel hooks.  The expected values are a restatement of the documented rule, not of the C code: S(K, N)
is the smallest S of {1, 2, 4, 8, 16} with ceil(N / 32) * S >= the family's fill constant, capped by K / 64 whole pairs, and
the split form runs up to the family's row threshold.  The three families read one policy function from one record each, so
the last two tests move one family's hooks and look at the other two."""
import pytest

from test_nf4_cpu import lib  # noqa: F401

# family -> (fill waves, row threshold), from the comments of the FQL_*_LINEAR_FILL_WAVES / _DECODE_MAX_ROWS constants
FAMILIES = {"mx4": (640, 16), "nvfp4": (720, 32), "lut4": (1280, 64)}
GROUPED_DECODE_MAX_ROWS = 512              # the one-wave decode kernel of the MXFP4 and NVFP4 grouped pair (no code-book twin)
# (K, N): the five shapes of DESIGN.md sections 36 and 43, the five of section 45, one pair and two pairs
SHAPES_36_43 = [(2880, 5120), (4096, 2880), (8192, 8192), (8192, 28672), (28672, 8192)]
SHAPES_45 = [(4096, 4096), (4096, 11008), (11008, 4096), (8192, 8192), (8192, 28672)]
SHAPES = sorted(set(SHAPES_36_43 + SHAPES_45)) + [(64, 4096), (128, 4096)]
# the one-row winners those sections record, which the constants were chosen to give
RECORDED = {"mx4": (SHAPES_36_43, [4, 8, 4, 1, 4]), "nvfp4": (SHAPES_36_43, [8, 8, 4, 1, 4]), "lut4": (SHAPES_45, [16, 4, 16, 8, 2])}


def policy_slices(fill, K, N):
    waves = -(-N // 32)
    S = next((s for s in (1, 2, 4, 8, 16) if waves * s >= fill), 16)
    while S > 1 and S > K // 64:
        S //= 2
    return S


def expected(family, T, K, N, fill=None, rows=None, forced=0):
    """What fql_tune_<family>_linear_kernel returns: slices << 8 | kernel (2 split form, 1 one-wave decode, 0 tile)."""
    fill = FAMILIES[family][0] if fill is None else fill
    rows = FAMILIES[family][1] if rows is None else rows
    split = 0 < T <= rows
    S = (forced or policy_slices(fill, K, N)) if split else 1
    if family == "lut4":                   # the decode form at S == 1 as well; above the threshold the tile kernel
        return (S << 8) | 2 if split else 1 << 8
    return (S << 8) | (2 if S > 1 else 1 if 0 < T <= GROUPED_DECODE_MAX_ROWS else 0)


def hook(lib, family):
    return getattr(lib, f"fql_tune_{family}_linear_kernel")


def set_rows(lib, family, rows):
    return getattr(lib, f"fql_tune_set_{family}_linear_decode_max_rows")(rows)


def set_slices(lib, family, slices):
    return getattr(lib, f"fql_tune_set_{family}_linear_slices")(slices)


@pytest.fixture
def defaults(lib):
    """The hooks at their documented defaults, asserted before and after (a negative threshold and 3 slices change nothing)."""
    def check():
        for family, (_, rows) in FAMILIES.items():
            assert set_rows(lib, family, -1) == rows and set_slices(lib, family, 3) == 0, family
        assert lib.fql_tune_set_mx4_decode_max_rows(-1) == GROUPED_DECODE_MAX_ROWS
        assert lib.fql_tune_set_nvfp4_decode_max_rows(-1) == GROUPED_DECODE_MAX_ROWS
    check()
    yield
    check()


@pytest.mark.parametrize("family", list(FAMILIES))
def test_policy_is_the_documented_rule(lib, defaults, family):
    rows = FAMILIES[family][1]
    for K, N in SHAPES:
        for T in (1, rows, rows + 1):
            assert hook(lib, family)(T, K, N) == expected(family, T, K, N), (family, T, K, N)
    shapes, winners = RECORDED[family]
    assert [hook(lib, family)(1, K, N) >> 8 for K, N in shapes] == winners
    assert hook(lib, family)(1, 64, 4096) >> 8 == 1 and hook(lib, family)(1, 128, 4096) >> 8 == 2   # never an empty slice
    assert hook(lib, family)(0, 8192, 8192) == expected(family, 0, 8192, 8192)


def _others_unmoved(lib, family, snapshot):
    for other in FAMILIES:
        if other != family:
            assert [hook(lib, other)(T, K, N) for T, K, N in snapshot[1]] == snapshot[0][other], (family, other)


@pytest.fixture
def snapshot(lib, defaults):
    points = [(T, K, N) for K, N in SHAPES for T in (1, 16, 17, 32, 33, 64, 65)]
    return {f: [hook(lib, f)(*p) for p in points] for f in FAMILIES}, points


@pytest.mark.parametrize("family", list(FAMILIES))
def test_forced_slices_move_one_family_only(lib, snapshot, family):
    for forced in (1, 2, 4, 8, 16):
        assert set_slices(lib, family, forced) == 0                          # (a setter returns the value it replaces)
        try:
            for K, N in SHAPES:
                for T in (1, FAMILIES[family][1] + 1):
                    assert hook(lib, family)(T, K, N) == expected(family, T, K, N, forced=forced), (family, forced, T, K, N)
            _others_unmoved(lib, family, snapshot)
        finally:
            assert set_slices(lib, family, 0) == forced


@pytest.mark.parametrize("family", list(FAMILIES))
def test_row_threshold_moves_one_family_only(lib, snapshot, family):
    default = FAMILIES[family][1]
    for rows in (0, 1, default + 7):
        assert set_rows(lib, family, rows) == default
        try:
            for K, N in SHAPES:
                for T in (1, rows, rows + 1):
                    assert hook(lib, family)(T, K, N) == expected(family, T, K, N, rows=rows), (family, rows, T, K, N)
            _others_unmoved(lib, family, snapshot)
        finally:
            assert set_rows(lib, family, default) == rows
