"""CPU-side tests (-m "not gpu") of the packed code rows of the fused NC kernels (include/mma_amd.h ABI 41: 2 bits per element in the
front of each row).  What ABI 41 does NOT change is pinned here: the row length mma_nc_crow_floats reports - still that of the
byte-per-element rows, 4 + n_sel * ceil(H/4) floats rounded up to 4 - and the entry points' requirements on the pitch `ldc`, refused on the
host before any launch.  The layout itself is tested on the GPU (test_nc_code_rows_gpu.py)."""
import pytest
import torch

from mma_amd import _lib
from mma_amd import functional as Fn
from test_nc_bf16_host import _refusal

WIDTHS = [1, 3, 4, 5, 8, 20, 36, 128, 132]
MASK_SETS = [["sum", "mean"], ["max"], ["sum", "mean", "max", "min"], ["max", "max2", "max3", "max4", "min", "min2", "min3", "min4"],
             ["softmax", "min"]]
SEL_KINDS = ("max", "min", "softmax", "softmin")


def kinds_of(names):
    from oracle import nc_oracle as O
    return [Fn.KIND[O.AGGREGATORS[n][0]] for n in names]


def n_slots(names):
    return sum(n.rstrip("234") in SEL_KINDS for n in names)


def packed_bytes(H, names):
    """The live front of a row: the 16-byte header and, per code slot, 2 bits per element rounded up to 4 bytes."""
    return 16 + n_slots(names) * 4 * -(-H // 16)


def test_abi_version():
    assert _lib.ABI_VERSION >= 41


@pytest.mark.parametrize("names", MASK_SETS, ids="-".join)
@pytest.mark.parametrize("H", WIDTHS)
def test_row_length_is_unchanged(H, names):
    want = (4 + n_slots(names) * -(-H // 4) + 3) // 4 * 4
    assert Fn.crow_floats(H, kinds_of(names)) == want
    assert packed_bytes(H, names) <= 4 * want                  # the packed slots fit the front of the row at every shape
    if n_slots(names) == 0:
        assert want == 4 and packed_bytes(H, names) == 16      # the header alone


def test_row_length_at_the_flagship_shape():
    assert Fn.crow_floats(128, kinds_of(["sum", "mean", "max", "min"])) == 68          # 272 bytes, of which 80 are live
    assert packed_bytes(128, ["sum", "mean", "max", "min"]) == 80


def test_row_length_refuses_bad_arguments():
    assert _lib.query("mma_nc_crow_floats", 0, 1, [0]) == -1
    assert _lib.query("mma_nc_crow_floats", 4, 9, [0] * 9) == -1
    assert _lib.query("mma_nc_crow_floats", 4, 1, [9]) == -1


# the arguments of test_nc_bf16_host: H = 4, [sum, max] -> rows of 8 floats
@pytest.mark.parametrize("name", ["mma_nc_fused_fwd", "mma_nc_fused_fwd_h"])
def test_forward_refuses_a_short_or_unaligned_code_row(name):
    for over in (dict(ldc=4), dict(ldc=7), dict(ldc=9), dict(ldc=10), dict(crow=torch.zeros(4 * 8 + 4)[1:], ldc=8)):
        assert "crow needs a 16-byte aligned pitch >= 8 floats" in _refusal(name, **over), over


@pytest.mark.parametrize("name", ["mma_nc_fused_bwd", "mma_nc_fused_bwd_h"])
def test_backward_refuses_a_short_code_row(name):
    assert "ldc=4 < 8" in _refusal(name, ldc=4)
    assert "ldc=7 < 8" in _refusal(name, ldc=7)


def test_node_backward_refuses_a_short_or_unaligned_code_row():
    N, H, K = 4, 4, 2
    f = lambda *s: torch.zeros(*s, dtype=torch.float32)
    vals = dict(g=f(N, H), g_kstride=0, ldgr=H, sel=None, T=f(N, K * H), ldt=K * H, rowptr=torch.zeros(N + 1, dtype=torch.int32), gs=None,
                ldgs=K * H, crow=f(N, 8), ldc=8, gP=f(N, K * H), ldgp=K * H, gxs=f(N, H), ldgx=H, row_max=None, N=N, H=H, K=K,
                kind_host=[0, 2], stream=None)
    for over in (dict(ldc=4), dict(ldc=9), dict(crow=f(4 * 8 + 4)[1:])):
        args = dict(vals, **over)
        with pytest.raises(_lib.MMALibraryError, match="crow needs a 16-byte aligned pitch >= 8 floats"):
            _lib.call("mma_nc_bwd_node", *[args[n] for _, _, n in _lib._abi.FUNCTIONS["mma_nc_bwd_node"][1]])
