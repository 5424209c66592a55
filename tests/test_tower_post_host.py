"""CPU-side tests (-m "not gpu") of the post-NN entry points (mma_amd/csrc/tower_post.hip: K13, K14, K15, K16, the scaler table, the
partial-tile reduction and the size queries): a valid argument set, one argument made wrong, and the text of the refusal.  Every
MMA_REQUIRE of that file comes before its launch, so host tensors stand in for device memory and no GPU is needed to see a refusal (the
pattern of tests/test_train_step_host.py).  No call here is left valid with N > 0: that would be a launch."""
import pytest
import torch

from mma_amd import _lib

N, T, KF, S, O = 70, 2, 36, 3, 15
K, OL = 36, 45                                  # the plain skinny Linear: K inputs, OL outputs (three 16-row tiles)
KFP = 64                                        # mma_tower_post_kfp(36)


def _f(*s):
    return torch.zeros(*s, dtype=torch.float32)


def _misaligned(n):
    """n floats that start 4 bytes past a 16-byte boundary."""
    buf = _f(n + 4)
    off = (16 - buf.data_ptr() % 16) // 4 % 4 + 1
    t = buf[off:off + n]
    assert t.data_ptr() % 16 == 4
    return t


def _values():
    return dict(
        agg=_f(N, T * KF), lda=T * KF, pre=_f(N, 8), Wa=_f(T * KFP * S * 16), Wb=_f(T * S * 16 * (KFP + 16)), y=_f(N, T * O), ldy=T * O,
        N=N, T=T, KF=KF, S=S, O=O, scaler_host=[0, 1, 3], avg_log=1.3, avg_lin=2.2, stream=None,
        gy=_f(N, T * O), ldg=T * O, gagg=_f(N, T * KF), gys=None, ldgs=0,
        part=_f(_lib.query("mma_tower_post_gw_chunks", N, T) * T * S * 16 * 48), n_chunks=_lib.query("mma_tower_post_gw_chunks", N, T),
        gWo=_f(T, O, S * KF), rowptr=torch.zeros(N + 1, dtype=torch.int32), Wo=_f(T, O, S * KF),
        # K16
        x=_f(N, K), ldx=K, bias=_f(OL), addend=None, ldadd=0, K=K, gx=_f(N, K), W=_f(OL, K), gw=_f(OL, K), gb=_f(OL), n_part=0)


def _args(name, over):
    vals = _values()
    if name.startswith("mma_skinny"):
        vals.update(O=OL, y=_f(N, OL), ldy=OL, gy=_f(N, OL), ldg=OL, Wa=_f(KFP * 48), Wb=_f(48 * (KFP + 16)))
        vals.update(n_part=_lib.query("mma_skinny_linear_gw_part", N, K, OL))
        vals.update(part=_f(max(vals["n_part"], 1)))
    vals.update(over)
    return [vals[n] for _, _, n in _lib._abi.FUNCTIONS[name][1]]


def _refusal(name, **over):
    with pytest.raises(_lib.MMALibraryError) as e:
        _lib.call(name, *_args(name, over))
    got = str(e.value)
    assert "%s failed (code 1)" % name in got, got
    return got


def _passes_without_a_launch(name, **over):
    _lib.call(name, *_args(name, over))                       # return code 0: call() raises on anything else


TOWER = ["mma_tower_post_fwd", "mma_tower_post_bwd", "mma_tower_post_gw"]
LIMITS = [
    ("KF513", dict(KF=513, lda=T * 513), "KF=513 S=3 O=15 unsupported (KF <= 512, S <= 5, O <= 16)"),
    ("S6", dict(S=6, scaler_host=[0] * 6), "S=6 O=15 unsupported"),
    ("O17_with_scaler_codes", dict(O=17, ldy=T * 17, ldg=T * 17), "S=3 O=17 unsupported"),
    ("T0", dict(T=0), "T=0 KF=36"),
    ("N_negative", dict(N=-1), "N=-1 T=2"),
    ("scaler_code_5", dict(scaler_host=[0, 5, 3]), "scaler[1]=5 is not an MMA_SC_* code"),
]


@pytest.mark.parametrize("name", TOWER)
@pytest.mark.parametrize("over,text", [c[1:] for c in LIMITS], ids=[c[0] for c in LIMITS])
def test_post_fill_limits(name, over, text):
    """post_fill(): the limits every tower entry point shares, checked first."""
    assert text in _refusal(name, **over)


def test_the_scaler_table_shares_the_limits():
    assert "S=6 O=1 unsupported" in _refusal("mma_tower_post_pre", S=6, scaler_host=[0] * 6)
    assert "scaler[2]=9 is not an MMA_SC_* code" in _refusal("mma_tower_post_pre", scaler_host=[0, 1, 9])
    assert "N=-1 " in _refusal("mma_tower_post_pre", N=-1)
    assert "NULL scaler codes" in _refusal("mma_tower_post_pre", scaler_host=None)
    assert "NULL argument" in _refusal("mma_tower_post_pre", rowptr=None)
    _passes_without_a_launch("mma_tower_post_pre", N=0, rowptr=None, pre=None)


PITCH = "NULL / misaligned argument or row pitch too small"
FWD = [
    ("lda_below_T_KF", dict(lda=T * KF - 1), PITCH),
    ("ldy_below_T_O", dict(ldy=T * O - 1), PITCH),
    ("Wa_not_16_byte_aligned", dict(Wa=_misaligned(T * KFP * S * 16)), PITCH),
    ("NULL_agg", dict(agg=None), PITCH),
    ("NULL_scaler_codes", dict(scaler_host=None), "NULL scaler codes"),
    ("KF385_S5_does_not_fit", dict(KF=385, lda=T * 385, S=5, scaler_host=[0, 1, 2, 3, 4]), "(167936 bytes with the tiles) do not fit the LDS"),
    ("KF481_S4_does_not_fit", dict(KF=481, lda=T * 481, S=4, scaler_host=[0, 1, 2, 3]), "(165888 bytes with the tiles) do not fit the LDS"),
]


@pytest.mark.parametrize("over,text", [c[1:] for c in FWD], ids=[c[0] for c in FWD])
def test_tower_post_fwd_refusals(over, text):
    assert text in _refusal("mma_tower_post_fwd", **over)


BWD = [
    ("lda_below_T_KF", dict(lda=T * KF - 1), PITCH),
    ("ldg_below_T_O", dict(ldg=T * O - 1), PITCH),
    ("Wb_not_16_byte_aligned", dict(Wb=_misaligned(T * S * 16 * (KFP + 16))), PITCH),
    ("NULL_gagg", dict(gagg=None), PITCH),
    ("NULL_scaler_codes", dict(scaler_host=None), "NULL scaler codes"),
    ("gys_pitch_below_T_S_16", dict(gys=_f(N, T * S * 16), ldgs=T * S * 16 - 1), "gys needs a pitch >= T*S*16 floats"),
    ("KF385_S5_does_not_fit", dict(KF=385, lda=T * 385, S=5, scaler_host=[0, 1, 2, 3, 4]), "(173056 bytes with the tiles) do not fit the LDS"),
    ("KF481_S4_does_not_fit", dict(KF=481, lda=T * 481, S=4, scaler_host=[0, 1, 2, 3]), "(169984 bytes with the tiles) do not fit the LDS"),
]


@pytest.mark.parametrize("over,text", [c[1:] for c in BWD], ids=[c[0] for c in BWD])
def test_tower_post_bwd_refusals(over, text):
    assert text in _refusal("mma_tower_post_bwd", **over)


GW = [
    ("lda_below_T_KF", dict(lda=T * KF - 1), "NULL argument or row pitch too small"),
    ("ldg_below_T_O", dict(ldg=T * O - 1), "NULL argument or row pitch too small"),
    ("NULL_part", dict(part=None), "NULL argument or row pitch too small"),
    ("one_chunk_too_many", dict(n_chunks=2), "n_chunks=2, expected mma_tower_post_gw_chunks(N, T)=1"),
    ("no_chunks", dict(n_chunks=0), "n_chunks=0, expected mma_tower_post_gw_chunks(N, T)=1"),
]


@pytest.mark.parametrize("over,text", [c[1:] for c in GW], ids=[c[0] for c in GW])
def test_tower_post_gw_refusals(over, text):
    assert text in _refusal("mma_tower_post_gw", **over)


def test_gw_chunk_count_follows_the_plan_variable(monkeypatch):
    """The n_chunks check asks the same query the caller did - under MMA_POST_GW_WAVES (read per call) as well."""
    monkeypatch.setenv("MMA_POST_GW_WAVES", "64")
    assert _lib.query("mma_tower_post_gw_chunks", 4097, 2) == 6
    assert "n_chunks=17, expected mma_tower_post_gw_chunks(N, T)=6" in _refusal("mma_tower_post_gw", N=4097, n_chunks=17)


REDUCE = [
    ("n_chunks_0", dict(n_chunks=0), "n_chunks=0 T=2 S=3 O=15 KF=36 unsupported (n_chunks <= 1024: mma_col_sum's single-pass order)"),
    ("n_chunks_1025", dict(n_chunks=1025), "n_chunks=1025 T=2"),
    ("O17", dict(O=17), "O=17 KF=36 unsupported"),
    ("NULL_gWo", dict(gWo=None), "NULL argument"),
    ("short_matrix_order", dict(n_chunks=257, T=1, S=1, KF=4, O=3), "n_chunks=257 with 256 columns: mma_col_sum sums this shape in its short-matrix order"),
    ("short_matrix_order_at_2048_columns", dict(n_chunks=257, T=2, S=1, KF=64, O=3), "n_chunks=257 with 2048 columns"),
]


@pytest.mark.parametrize("over,text", [c[1:] for c in REDUCE], ids=[c[0] for c in REDUCE])
def test_tower_post_gw_reduce_refusals(over, text):
    assert text in _refusal("mma_tower_post_gw_reduce", **over)


@pytest.mark.parametrize("name", TOWER)
def test_an_empty_graph_passes_without_a_launch(name):
    _passes_without_a_launch(name, N=0, n_chunks=0, agg=None, gy=None, y=None, gagg=None, part=None)


def test_weight_layout_refusals():
    assert "T=2 O=17 S=3 KF=36 unsupported" in _refusal("mma_tower_post_weights", O=17)
    assert "NULL argument" in _refusal("mma_tower_post_weights", Wo=None)
    assert "O=81 K=36 unsupported" in _refusal("mma_skinny_linear_weights", O=81)
    assert "O=45 K=513 unsupported" in _refusal("mma_skinny_linear_weights", K=513)


SKINNY_FWD = [
    ("O81", dict(O=81, ldy=81), "O=81 unsupported (<= 80)"),
    ("K513", dict(K=513, ldx=513), "T=1 KF=513 S=3 O=45 unsupported"),
    ("ldx_below_K", dict(ldx=K - 1), PITCH),
    ("ldy_below_O", dict(ldy=OL - 1), PITCH),
    ("Wa_not_16_byte_aligned", dict(Wa=_misaligned(KFP * 48)), PITCH),
    ("ldadd_below_O", dict(addend=_f(N, OL), ldadd=OL - 1), "ldadd=44 < O"),
    ("N_negative", dict(N=-1), "N=-1 T=1"),
]


@pytest.mark.parametrize("over,text", [c[1:] for c in SKINNY_FWD], ids=[c[0] for c in SKINNY_FWD])
def test_skinny_linear_fwd_refusals(over, text):
    assert text in _refusal("mma_skinny_linear_fwd", **over)


SKINNY_DX = [
    ("O81", dict(O=81, ldg=81), "O=81 unsupported (<= 80)"),
    ("K513", dict(K=513, ldx=513), "T=1 KF=513 S=3 O=45 unsupported"),
    ("ldx_below_K", dict(ldx=K - 1), PITCH),
    ("ldg_below_O", dict(ldg=OL - 1), PITCH),
    ("Wb_not_16_byte_aligned", dict(Wb=_misaligned(48 * (KFP + 16))), PITCH),
]


@pytest.mark.parametrize("over,text", [c[1:] for c in SKINNY_DX], ids=[c[0] for c in SKINNY_DX])
def test_skinny_linear_bwd_dx_refusals(over, text):
    assert text in _refusal("mma_skinny_linear_bwd_dx", **over)


SKINNY_GW = [
    ("O81", dict(O=81, ldg=81), "O=81 K=36 unsupported (O <= 80, K <= 512)"),
    ("K513", dict(K=513, ldx=513), "O=45 K=513 unsupported"),
    ("N0", dict(N=0), "N=0 unsupported"),
    ("n_part_one_float_short", dict(n_part=48 * 48 - 1), "n_part=2303, expected mma_skinny_linear_gw_part(N, K, O)=2304"),
    ("ldx_below_K", dict(ldx=K - 1), "NULL argument or row pitch too small"),
    ("ldg_below_O", dict(ldg=OL - 1), "NULL argument or row pitch too small"),
    ("NULL_gw", dict(gw=None), "NULL argument or row pitch too small"),
]


@pytest.mark.parametrize("over,text", [c[1:] for c in SKINNY_GW], ids=[c[0] for c in SKINNY_GW])
def test_skinny_linear_gw_refusals(over, text):
    assert text in _refusal("mma_skinny_linear_gw", **over)


def test_skinny_linear_of_no_rows_passes_without_a_launch():
    _passes_without_a_launch("mma_skinny_linear_fwd", N=0, x=None, y=None)
    _passes_without_a_launch("mma_skinny_linear_bwd_dx", N=0, gy=None, gx=None)


def test_size_queries():
    q = _lib.query
    assert [q("mma_tower_post_kfp", kf) for kf in (0, -3, 1, 32, 33, 512)] == [-1, -1, 32, 32, 64, 512]
    # (N, K, O) outside the kernel's limits: no workspace
    assert [q("mma_skinny_linear_gw_part", *a) for a in ((0, 36, 45), (-1, 36, 45), (70, 0, 45), (70, 513, 45), (70, 36, 0), (70, 36, 81))] == [0] * 6
    assert q("mma_skinny_linear_gw_part", 70, 36, 45) == 1 * 48 * 48          # one chunk, S*16 rows, round_up(K + 1, 16) columns
    assert q("mma_skinny_linear_gw_part", 70, 47, 45) == 1 * 48 * 48 and q("mma_skinny_linear_gw_part", 70, 48, 45) == 1 * 48 * 64     # the ones column
    assert [q("mma_tower_post_gw_chunks", *a) for a in ((0, 2), (-1, 2), (5, 0))] == [0, 0, 0]


FITS = [(480, 4, 1), (481, 4, 0), (384, 5, 1), (385, 5, 0), (512, 3, 1), (513, 1, 0), (4, 6, 0), (0, 1, 0), (4, 0, 0), (512, 1, 1), (1, 5, 1)]


@pytest.mark.parametrize("kf,s,want", FITS, ids=["%d_%d" % c[:2] for c in FITS])
def test_tower_post_fits_at_its_corners(kf, s, want):
    assert _lib.query("mma_tower_post_fits", kf, s) == want


@pytest.mark.parametrize("waves,want", [(None, (17, 129)), ("64", (6, 16)), ("63", (17, 129)), ("2048", (17, 258))], ids=["unset", "64", "63_is_ignored", "2048"])
def test_gw_chunks_under_the_plan_variable(waves, want, monkeypatch):
    """mma_tower_post_gw_chunks for the shapes of the K15 tests, (4097, T = 2) and (66000, T = 1): 1024 wavefronts over the towers by
    default, ranges of a multiple of 64 nodes, four ranges per chunk.  64 waves: 32 per tower, 192-node ranges, 22 of them, 6 chunks;
    2048 waves at (66000, 1): 64-node ranges, 1032 of them, 258 chunks - past the 256 the single-launch reduction takes."""
    if waves is None:
        monkeypatch.delenv("MMA_POST_GW_WAVES", raising=False)
    else:
        monkeypatch.setenv("MMA_POST_GW_WAVES", waves)
    assert (_lib.query("mma_tower_post_gw_chunks", 4097, 2), _lib.query("mma_tower_post_gw_chunks", 66000, 1)) == want
