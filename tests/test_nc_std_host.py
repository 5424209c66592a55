"""CPU-side tests (-m "not gpu") of the std aggregator's entry points (include/mma_amd.h ABI 37, csrc/nc_moments.hip): bad arguments
are refused on the host through the library's error path, before any launch - no GPU is needed to see it."""
import pytest
import torch

from mma_amd import _lib


def _fwd_args(N=4, E=4, H=4, items="ok", hubs=None, n_hubs=0, partial=None, n_slots=0):
    f = lambda *s: torch.zeros(*s, dtype=torch.float32)
    i = lambda *s: torch.zeros(*s, dtype=torch.int32)
    its = i(N, 4) if items == "ok" else items
    return [f(N, H), H, f(N, H), H, f(N, H), H, i(N + 1), i(max(E, 1)), its, N, N, hubs, n_hubs, partial, n_slots,
            f(N, H), H, f(N, 3 * H), 3 * H, N, E, H, [0], 0, 0, 0, None, 0, None, None]


def _bwd_args(N=4, E=4, H=4, items="ok", hubs=None, n_hubs=0, partial=None, n_slots=0):
    f = lambda *s: torch.zeros(*s, dtype=torch.float32)
    i = lambda *s: torch.zeros(*s, dtype=torch.int32)
    its = i(N, 4) if items == "ok" else items
    return [f(N, H), H, f(N, H), H, f(N, H), H, f(N, H), H, f(N, 3 * H), 3 * H, f(N, H), H, f(N, H), H, N,
            i(max(E, 1)), i(max(E, 1)), its, N, N, hubs, n_hubs, partial, n_slots, f(N, H), H, f(N, H), H,
            N, E, H, [0], 0, 0, 0, None, 0, None, None]


@pytest.mark.parametrize("name,args", [("mma_nc_std_fwd", _fwd_args), ("mma_nc_std_bwd", _bwd_args)])
def test_std_entry_points_refuse_bad_arguments_on_the_host(name, args):
    assert len(args()) == len(_lib.PROTOTYPES[name])
    with pytest.raises(_lib.MMALibraryError, match="NULL argument"):
        _lib.call(name, *args(items=None))
    base = torch.zeros(12, dtype=torch.int32)
    assert base.data_ptr() % 16 == 0
    with pytest.raises(_lib.MMALibraryError, match="16-byte aligned"):
        _lib.call(name, *args(hubs=base[1:5], n_hubs=1, partial=torch.zeros(64), n_slots=1))       # 4 bytes off
    with pytest.raises(_lib.MMALibraryError, match="hub slots without"):
        _lib.call(name, *args(n_slots=3))
    for H in (0, -4):
        with pytest.raises(_lib.MMALibraryError, match="H=%d unsupported" % H):
            _lib.call(name, *_with_h(args(), name, H))
    with pytest.raises(_lib.MMALibraryError, match="pitch"):
        a = args()
        a[1] = 2                                                                                    # ldx < H
        _lib.call(name, *a)


def _with_h(a, name, H):
    """The argument list with the H parameter replaced (the buffers keep their shapes: the check fires before they are looked at)."""
    names = [n for _, _, n in _lib._abi.FUNCTIONS[name][1]]
    a = list(a)
    a[names.index("H")] = H
    return a


def test_std_refuses_bad_codes():
    a = _fwd_args()
    names = [n for _, _, n in _lib._abi.FUNCTIONS["mma_nc_std_fwd"][1]]
    a[names.index("act_host")] = [7]
    with pytest.raises(_lib.MMALibraryError, match="act=7"):
        _lib.call("mma_nc_std_fwd", *a)
    a = _fwd_args()
    a[names.index("drop_mode")] = 2                       # EXPLICIT without a keep mask
    with pytest.raises(_lib.MMALibraryError, match="keep mask"):
        _lib.call("mma_nc_std_fwd", *a)


def test_std_refuses_cpu_tensors_and_the_sharded_layer_refuses_std():
    from mma_amd import functional as Fn
    from mma_amd.sharded import ShardedMMA
    x = torch.zeros(4, 4)
    with pytest.raises(_lib.MMALibraryError, match="GPU only"):
        Fn.nc_std_aggregate(x, x, x, None)
    with pytest.raises(NotImplementedError, match="std"):
        ShardedMMA(None, "cpu", 4, 2, ["mean", "std"], {}, None, None, 0.0)
