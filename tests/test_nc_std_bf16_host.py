"""CPU-side tests (-m "not gpu") of the std aggregator's bf16-table entry points (include/mma_amd.h ABI 40: mma_nc_std_fwd_h,
mma_nc_std_bwd_h; csrc/nc_moments.hip) and of the `logit_dtype` keyword of nc_std_aggregate: every bad argument the fp32 entry points
refuse on the host is refused by their bf16 twins with the same text, before any launch - no GPU is needed to see it."""
import ctypes

import pytest
import torch

from mma_amd import _lib
from mma_amd import functional as Fn

N, E, H = 4, 4, 4
TWINS = [("mma_nc_std_fwd", "mma_nc_std_fwd_h"), ("mma_nc_std_bwd", "mma_nc_std_bwd_h")]


def _values(table_dtype):
    f = lambda *s: torch.zeros(*s, dtype=torch.float32)
    i = lambda *s: torch.zeros(*s, dtype=torch.int32)
    t = lambda *s: torch.zeros(*s, dtype=table_dtype)
    return dict(
        x=f(N, H), ldx=H, P=t(N, H), ldp=H, Q=t(N, H), ldq=H, rowptr=i(N + 1), col=i(E), items=i(N, 4), n_items=N, n_wave_items=N,
        hubs=None, n_hubs=0, partial=None, n_slots=0, m=f(N, H), ldms=H, saved=f(N, 3 * H), ldt=3 * H,
        N=N, E=E, H=H, act_host=[0], drop_mode=0, drop_thr=0, seed=0, seed_dev=None, drop_edge_base=0, keep=None, stream=None,
        # the backward's own
        g=f(N, H), ldg=H, gr=f(N, H), ldgr=H, gP=f(N, H), ldgp=H, n_targets=N, t_col=i(E), t_eid=i(E), gQ=f(N, H), ldgq=H, gx=f(N, H), ldgx=H)


def _args(name, **over):
    vals = _values(torch.bfloat16 if name.endswith("_h") else torch.float32)
    vals.update(over)
    return [vals[n] for _, _, n in _lib._abi.FUNCTIONS[name][1]]


def _refusal(name, **over):
    with pytest.raises(_lib.MMALibraryError) as e:
        _lib.call(name, *_args(name, **over))
    return str(e.value).replace(name, "<entry>")


def test_the_new_entry_points_are_declared_exported_and_bound():
    assert _lib.ABI_VERSION >= 40
    L = ctypes.CDLL(_lib.LIB_PATH)
    for f32, h in TWINS:
        assert h in _lib._abi.FUNCTIONS and h in _lib.PROTOTYPES
        # same parameter lists: only the storage of P and Q differs (the bindings see both as pointers)
        assert _lib._abi.FUNCTIONS[f32] == _lib._abi.FUNCTIONS[h]
        assert len(_args(h)) == len(_lib.PROTOTYPES[h])
        assert getattr(L, h) is not None                     # exported by the library (AttributeError otherwise)
        if _lib.ops():
            assert hasattr(_lib.ops(), h)                    # and registered as a torch op


BAD = [
    (dict(N=-1), "out of int32 range"),
    (dict(H=0), "H=0 unsupported"),
    (dict(H=-4), "H=-4 unsupported"),
    (dict(ldx=2), "pitch too small"),
    (dict(ldp=H - 1), "pitch too small"),
    (dict(ldq=1), "pitch too small"),
    (dict(ldp=1 << 31), "pitch out of range"),
    (dict(n_items=-1), "negative or oversize item counts"),
    (dict(n_slots=3), "hub slots without"),
    (dict(items=None), "NULL argument"),
    (dict(P=None), "NULL argument"),
    (dict(Q=None), "NULL argument"),
    (dict(act_host=[7]), "act=7"),
    (dict(drop_mode=2), "keep mask"),
    (dict(drop_mode=7), "drop_mode 7 unknown"),
]


@pytest.mark.parametrize("f32,h", TWINS)
@pytest.mark.parametrize("over,text", BAD, ids=["%d-%s" % (n, "-".join(sorted(o))) for n, (o, _) in enumerate(BAD)])
def test_h_entry_points_refuse_what_their_fp32_twins_refuse(f32, h, over, text):
    want, got = _refusal(f32, **over), _refusal(h, **over)
    assert got == want                                      # the same check, the same text
    assert text in got, got


@pytest.mark.parametrize("f32,h", TWINS)
def test_h_entry_points_refuse_misaligned_item_lists(f32, h):
    base = torch.zeros(12, dtype=torch.int32)
    assert base.data_ptr() % 16 == 0
    over = dict(hubs=base[1:5], n_hubs=1, partial=torch.zeros(64, dtype=torch.float64), n_slots=1)      # 4 bytes off
    assert _refusal(h, **over) == _refusal(f32, **over) and "16-byte aligned" in _refusal(h, **over)


@pytest.mark.parametrize("f32,h", TWINS)
def test_h_entry_points_refuse_a_table_at_an_odd_address(f32, h):
    raw = torch.zeros(2 * N * H + 16, dtype=torch.uint8)
    assert raw.data_ptr() % 2 == 0
    odd = raw[1:1 + 2 * N * H]                               # a bf16 table cannot start here: its elements would straddle 2-byte units
    for which in ("P", "Q"):
        assert "odd address" in _refusal(h, **{which: odd})
    _lib.call(h, *_args(h, P=odd, n_items=0))                # nothing to do: no launch, no error - as in the fp32 twin
    _lib.call(f32, *_args(f32, n_items=0))


def test_nc_std_aggregate_refuses_mixed_and_widened_tables():
    x, p32, pbf = torch.zeros(N, H), torch.zeros(N, H), torch.zeros(N, H, dtype=torch.bfloat16)
    # the storage checks come before the GPU check: a CPU tensor is enough to see them
    for P, Q in ((p32, pbf), (pbf, p32)):
        with pytest.raises(ValueError, match="share a dtype"):
            Fn.nc_std_aggregate(x, P, Q, None)
        with pytest.raises(ValueError, match="share a dtype"):
            Fn.nc_std_aggregate(x, P, Q, None, logit_dtype=torch.bfloat16)
        with pytest.raises(ValueError, match="share a dtype"):
            Fn.nc_std_fwd_launch(x, P, Q, None, Fn.ACT_SIGMOID, Fn.DropoutSpec(0.0), True)
        with pytest.raises(ValueError, match="share a dtype"):
            Fn.nc_std_bwd_launch(x, P, Q, x, None, None, Fn.ACT_SIGMOID, Fn.DropoutSpec(0.0), None, None, None)
    with pytest.raises(ValueError, match="cannot be widened"):
        Fn.nc_std_aggregate(x, pbf, pbf, None, logit_dtype=torch.float32)
    with pytest.raises(ValueError, match="logit_dtype"):
        Fn.nc_std_aggregate(x, p32.half(), p32.half(), None)
    with pytest.raises(ValueError, match="logit_dtype"):
        Fn.nc_std_aggregate(x, p32, p32, None, logit_dtype=torch.float16)
    with pytest.raises(_lib.MMALibraryError, match="GPU only"):          # a well-formed call on CPU tensors is refused as ever
        Fn.nc_std_aggregate(x, pbf, pbf, None, logit_dtype=torch.bfloat16)


def test_check_logit_dtype_errors_are_unchanged():
    assert Fn.check_logit_dtype(torch.float32) == torch.float32 and Fn.check_logit_dtype(torch.bfloat16) == torch.bfloat16
    for bad in (torch.float16, torch.float64, "bf16", None):
        with pytest.raises(ValueError, match=r"logit_dtype has to be torch.float32 or torch.bfloat16, but got"):
            Fn.check_logit_dtype(bad)
    with pytest.raises(ValueError, match="logit_dtype"):
        Fn.nc_std_local(torch.zeros(4, 4), torch.zeros(8, 4), None, logit_dtype=torch.float16)


def _layer(aggs, **kw):
    import mma_amd
    from golden.inputs import ALL_MASK_NAMES
    P = lambda *s: torch.nn.Parameter(torch.empty(*s))
    masks = [P(2 * H, H) for _ in ALL_MASK_NAMES]
    return mma_amd.MMA([[1], [0], [], [2]], "sigmoid", 2, H, 3, P(H, 3), P(3), *masks, 0.0, aggs, "cpu", **kw)


def test_strict_mode_and_the_sharded_layer_still_refuse_std():
    from mma_amd.sharded import ShardedMMA
    strict = _layer(["mean", "std"], logit_dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="std"):
        strict.learnable_std(torch.zeros(4, H), None)
    with pytest.raises(NotImplementedError, match="std"):
        ShardedMMA(None, "cpu", 4, 2, ["mean", "std"], {}, None, None, 0.0)
    with pytest.raises(_lib.MMALibraryError, match="GPU only"):          # the extension mode reaches the GPU check, whatever the table type
        _layer(["std"], logit_dtype=torch.bfloat16, strict_reference=False).learnable_std(torch.zeros(4, H), None)
