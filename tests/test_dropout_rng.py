"""Statistics of the counter-based dropout stream (oracle/dropout_rng.py = the numpy restatement of mma_amd/csrc/common.h's
drop_base_word / drop_mask_word / drop_low_word; the `-m gpu` tests check that the kernels' hash mode equals these masks bit for bit).

Round 3 derives the K masks' words from ONE full hash per (edge, feature quad).  A shared hash makes these checks necessary
(round-2 VERDICT item 4): the keep rate must be 1 - thr/256 within 3 sigma for every mask, and the masks k != k' of one edge
must be uncorrelated - tested on the keep bits themselves, on the XOR of two bytes of a word (the statistic that exposed the
rejected derivation r_k = fold16(h * M_k): 800 sigma), and between neighbouring edges and quads."""
import numpy as np
import pytest

from oracle.dropout_rng import keep_mask, mask_words

K, E, H = 8, 60000, 64
N_ELEM = E * H


@pytest.mark.parametrize("seed", [0, 0x0123456789ABCDEF, 2 ** 64 - 1])
@pytest.mark.parametrize("thr", [128, 192, 64, 13])
def test_keep_rate_and_mask_independence(seed, thr):
    keep = keep_mask(seed, thr, K, E, H).astype(np.float64)            # (K,E,H)
    p = 1.0 - thr / 256.0
    sigma = np.sqrt(p * (1 - p) / N_ELEM)
    rates = keep.reshape(K, -1).mean(1)
    # 3 sigma per mask is a 0.27 % event each; 8 masks x 12 cases: allow 3.7 sigma (1 in 4600) so the test is not flaky by design
    assert np.all(np.abs(rates - p) < 3.7 * sigma), (rates - p) / sigma
    assert abs(rates.mean() - p) < 3.0 * sigma / np.sqrt(K), (rates.mean() - p) / sigma * np.sqrt(K)
    c = keep.reshape(K, -1) - p
    corr = (c @ c.T) / N_ELEM / (p * (1 - p))
    off = np.abs(corr[~np.eye(K, dtype=bool)])
    assert off.max() * np.sqrt(N_ELEM) < 4.5, "masks k != k' of one edge are correlated: %.2f sigma" % (off.max() * np.sqrt(N_ELEM))


def test_bytes_of_all_masks_of_a_word_are_pairwise_independent():
    """All 8 masks x 4 bytes of one (edge, quad): 32 Bernoulli variables, 496 pairs, none correlated (p = 0.5 and p = 0.75)."""
    for thr in (128, 64):
        keep = keep_mask(7, thr, K, E, H).astype(np.float64)
        p = 1.0 - thr / 256.0
        v = keep.reshape(K, E, H // 4, 4).transpose(1, 2, 0, 3).reshape(-1, K * 4) - p
        cc = (v.T @ v) / v.shape[0] / (p * (1 - p))
        off = np.abs(cc[~np.eye(K * 4, dtype=bool)])
        assert off.max() * np.sqrt(v.shape[0]) < 4.8, off.max() * np.sqrt(v.shape[0])


def test_xor_of_two_bytes_is_independent_across_masks():
    """(keep_k[i] ^ keep_k[j]) against (keep_k'[i] ^ keep_k'[j]) at p = 0.5: the second-order statistic that a one-round
    derivation of the masks' words from a shared hash fails by hundreds of sigma."""
    kb = keep_mask(11, 128, K, E, H).reshape(K, E, H // 4, 4).astype(np.int8)
    worst = 0.0
    for i in range(4):
        for j in range(i + 1, 4):
            x = (kb[..., i] ^ kb[..., j]).reshape(K, -1).astype(np.float64) - 0.5
            cx = (x @ x.T) / x.shape[1] / 0.25
            worst = max(worst, np.abs(cx[~np.eye(K, dtype=bool)]).max() * np.sqrt(x.shape[1]))
    assert worst < 5.0, worst


def test_neighbouring_edges_and_quads_are_independent():
    keep = keep_mask(3, 128, K, E, H).astype(np.float64) - 0.5
    n = (E - 1) * H
    adj_e = np.abs((keep[:, :-1] * keep[:, 1:]).mean((1, 2)) / 0.25) * np.sqrt(n)
    q = keep.reshape(K, E, H // 4, 4)
    adj_q = np.abs((q[:, :, :-1] * q[:, :, 1:]).mean((1, 2, 3)) / 0.25) * np.sqrt(E * (H // 4 - 1) * 4)
    assert adj_e.max() < 4.5 and adj_q.max() < 4.5, (adj_e, adj_q)


def test_words_are_a_function_of_the_global_edge_id_and_the_seed():
    """A shard generates the bits of ITS edges from their global positions (`edge_ids`): sharded == single-GPU for one seed;
    mask 0's word is the base hash itself (the graph-regression kernels, which have one mask, are unchanged by round 3)."""
    w = mask_words(42, 4, 1000, 16)
    part = mask_words(42, 4, 300, 16, edge_ids=np.arange(500, 800))
    assert np.array_equal(w[:, 500:800], part)
    assert not np.array_equal(mask_words(43, 4, 1000, 16), w)
    assert np.array_equal(mask_words(42, 1, 1000, 16)[0], w[0])
    assert len({w[k].tobytes() for k in range(4)}) == 4


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 64, 65, 200])
def test_seed_advance_is_splitmix64(n):
    """mma_seed_advance (the one captured launch that redraws a layer's dropout seeds per replay) against its restatement: part of a
    64-thread block, one full block, one block and a thread, several blocks."""
    import torch
    from mma_amd import functional as Fn
    from oracle.dropout_rng import splitmix64
    ds = Fn.DeviceSeeds(n, torch.device("cuda:0"))
    states = [int(v) & ((1 << 64) - 1) for v in ds.buf[n:].tolist()]
    for _ in range(3):
        got = [int(v) & ((1 << 64) - 1) for v in ds.advance().tolist()]
        nxt = [splitmix64(s) for s in states]
        states = [a for a, _ in nxt]
        assert got == [b for _, b in nxt]
        assert [int(v) & ((1 << 64) - 1) for v in ds.buf[n:].tolist()] == states
    assert len(set(got)) == n


def test_hash_dropout_applies_any_probability_to_16_bits():
    """Round-4 VERDICT item 7: the reference's F.dropout takes any p (layers.py:219, train.py:27).  The kernels compare a 16-bit hash value
    with thr = round(65536 p): |p_applied - p| <= 2^-17 < 8e-6 for EVERY p, no warning path, the README's 0.5 / 0.75 exact."""
    import warnings
    from mma_amd import functional as Fn
    from oracle.dropout_rng import threshold16
    rng = np.random.default_rng(0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                       # nothing may warn
        for p in [0.5, 0.75, 0.25, 0.3, 0.33, 0.1, 0.6, 0.05, 1e-4, 0.999, 1 / 3] + rng.random(200).tolist():
            d = Fn.DropoutSpec(p, seed=1)
            assert abs(d.p_applied - p) <= 8e-6 and d.thr == threshold16(p) and d.mode == Fn.DROP_HASH, (p, d.p_applied)
        assert Fn.DropoutSpec(0.5, seed=1).thr == 32768 and Fn.DropoutSpec(0.75, seed=1).p_applied == 0.75
        assert Fn.DropoutSpec(0.0).p_applied == 0.0 and Fn.DropoutSpec(0.0).mode == Fn.DROP_NONE
    assert not hasattr(Fn, "_WARNED_P")
    with pytest.raises(ValueError):
        Fn.DropoutSpec(1.0)


@pytest.mark.parametrize("p", [0.6, 0.3, 0.1, 0.9373, 0.0042])
def test_keep_rate_and_independence_with_16_bit_thresholds(p):
    """The 16-bit form (thr16 no multiple of 256: the low byte of a value comes from a SECOND word folded from the same hash): keep rate
    1 - thr16/65536 within 3.7 sigma per mask, masks uncorrelated, the 32 decisions of one (edge, quad) pairwise uncorrelated - and the
    rate really is the 16-bit one (the 8-bit neighbours thr16 >> 8 and (thr16 >> 8) + 1 are rejected where they are > 6 sigma away)."""
    from oracle.dropout_rng import keep_mask16, threshold16
    thr = threshold16(p)
    assert thr % 256 != 0
    keep = keep_mask16(0xFEEDFACE12345678, thr, K, E, H).astype(np.float64)
    q = 1.0 - thr / 65536.0
    sigma = np.sqrt(q * (1 - q) / N_ELEM)
    rates = keep.reshape(K, -1).mean(1)
    assert np.all(np.abs(rates - q) < 3.7 * sigma), (rates - q) / sigma
    assert abs(rates.mean() - q) < 3.0 * sigma / np.sqrt(K), (rates.mean() - q) / sigma * np.sqrt(K)
    for t8 in (thr >> 8, (thr >> 8) + 1):                                   # 1 - t8/256 is NOT the rate
        if abs((1.0 - t8 / 256.0) - q) > 6 * sigma / np.sqrt(K):
            assert abs(rates.mean() - (1.0 - t8 / 256.0)) > 3 * sigma / np.sqrt(K)
    c = keep.reshape(K, -1) - q
    corr = (c @ c.T) / N_ELEM / (q * (1 - q))
    assert np.abs(corr[~np.eye(K, dtype=bool)]).max() * np.sqrt(N_ELEM) < 4.5
    v = keep.reshape(K, E, H // 4, 4).transpose(1, 2, 0, 3).reshape(-1, K * 4) - q
    cc = (v.T @ v) / v.shape[0] / (q * (1 - q))
    assert np.abs(cc[~np.eye(K * 4, dtype=bool)]).max() * np.sqrt(v.shape[0]) < 4.8


def test_low_bytes_decide_only_on_a_high_byte_tie_and_are_uniform_there():
    """What the second word is for: among the elements whose HIGH byte equals thr16 >> 8 (1 in 256) the LOW byte decides, and there it
    must be uniform and uncorrelated with the neighbouring elements' decisions; a multiple of 256 reproduces the 8-bit masks bit for bit."""
    from oracle.dropout_rng import keep_mask16, low_words
    seed, thr = 99, (153 << 8) | 154                                          # p ~ 0.6
    assert np.array_equal(keep_mask16(seed, 128 * 256, K, 5000, H), keep_mask(seed, 128, K, 5000, H))
    r = mask_words(seed, K, E, H // 4)
    lo = low_words(seed, K, E, H // 4)
    for byte in range(4):
        hi_b = (r >> np.uint64(8 * byte)) & np.uint64(0xFF)
        lo_b = ((lo >> np.uint64(8 * byte)) & np.uint64(0xFF))[hi_b == np.uint64(thr >> 8)].astype(np.float64)
        n = lo_b.size
        assert n > 0.8 * K * E * (H // 4) / 256
        assert abs(lo_b.mean() - 127.5) < 4.5 * np.sqrt((256 ** 2 - 1) / 12.0 / n)            # uniform on 0..255: mean, and the kept share
        share = (lo_b >= (thr & 0xFF)).mean()
        ps = 1 - (thr & 0xFF) / 256.0
        assert abs(share - ps) < 4.5 * np.sqrt(ps * (1 - ps) / n)
    keep = keep_mask16(seed, thr, K, E, H)
    tie = (((r[:, :, :, None] >> (np.uint64(8) * np.arange(4, dtype=np.uint64))) & np.uint64(0xFF)) == np.uint64(thr >> 8)).reshape(K, E, H)
    nxt = np.roll(keep, -1, axis=2).astype(np.float64)[tie]                    # the neighbour element's decision, on the tie elements
    mine = keep.astype(np.float64)[tie]
    q = 1.0 - thr / 65536.0
    cov = ((mine - mine.mean()) * (nxt - q)).mean() / np.sqrt(mine.var() * q * (1 - q))
    assert abs(cov) * np.sqrt(mine.size) < 4.5, cov * np.sqrt(mine.size)
