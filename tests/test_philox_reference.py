"""CPU checks of tests/philox_models.py, the float64 model the GPU tests of test_gpu_philox.py compare the Philox kernels with: the published
Random123 known-answer vectors of philox4x32_10, the Box-Muller extreme words the GPU test feeds to set_randn, the counter words that keep
streams apart, and the model's own moments (so that the moments bound of test_posterior_qsample_randn is one the exact stream meets)."""
import numpy as np
import pytest

import philox_models as PM

# Random123 (kat_vectors, philox4x32 10): counter, key, output words
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_known_answer_vectors():
    for ctr, key, want in KAT:
        got = PM.philox4x32_10(*ctr, *key)
        assert tuple(int(w[0]) for w in got) == want, (ctr, key, [hex(int(w[0])) for w in got])
    # vectorised: the three at once give the same words
    got = PM.philox4x32_10(*[[k[0][i] for k in KAT] for i in range(4)], *[[k[1][i] for k in KAT] for i in range(2)])
    assert [tuple(int(w[j]) for w in got) for j in range(3)] == [k[2] for k in KAT]
    # and through the stream addressing: (seed 0, offset 0) is the first vector; the third one has counter words 2, 3 set, so only
    # its key and low counter words can be addressed: the stream's key / counter split is checked on a counter of the same form instead
    assert tuple(int(w) for w in PM.words(0, 0, 1)[0]) == KAT[0][2]
    seed, off = 0x299f31d0a4093822, 0x85a308d3243f6a88
    direct = PM.philox4x32_10(0x243f6a88, 0x85a308d3, 0, 0, 0xa4093822, 0x299f31d0)
    assert np.array_equal(PM.words(seed, off, 1)[0], np.array([w[0] for w in direct]))
    direct = PM.philox4x32_10(0x243f6a88, 0x85a308d3, 0x5eed, 0, 0xa4093822, 0x299f31d0)
    assert np.array_equal(PM.words(seed, off, 1, PM.DROPOUT_WORD)[0], np.array([w[0] for w in direct]))


def test_box_muller_extreme_words():
    """The counters of PM.EXTREMES have the stated top 24 bits at seed 0, and the model's normals there are what the limits say."""
    exact = {(17758991, 0): 0x00000079, (38471471, 0): 0xffffffec, (17169035, 1): 0x000000c8, (44150062, 1): 0xffffff44}
    for ctr, k, what in PM.EXTREMES:
        w = PM.words(0, ctr, 1)
        top = int(w[0, k]) >> 8
        assert top == (0 if what == "zero" else 0xFFFFFF), (ctr, k, hex(int(w[0, k])))
        if (ctr, k) in exact:
            assert int(w[0, k]) == exact[ctr, k]
        z, r = PM.box_muller(w)
        assert np.isfinite(z).all()
        u = PM.uniforms(w)[0, k]
        assert u == (2.0 ** -24 if what == "zero" else 1.0)
        pair = slice(0, 2) if k < 2 else slice(2, 4)
        if k in (0, 2):
            if what == "zero":  # the largest radius the generator can give: sqrt(48 ln 2)
                assert abs(r[0, k] - np.sqrt(48.0 * np.log(2.0))) < 1e-12
            else:
                assert (z[0, pair] == 0.0).all() and r[0, k] == 0.0
        elif what == "ones":  # angle 2 pi: (r, 0) up to the rounding of pi
            assert abs(z[0, pair][0] - r[0, k]) < 1e-12 and abs(z[0, pair][1]) < 1e-12


def test_counter_and_key_words_separate_the_streams():
    n = 64
    for seed, off in ((0, 0), (7, 5), (0xDEADBEEF12345678, 17 * 2 ** 28)):
        assert not (PM.words(seed, off, n // 4, PM.DROPOUT_WORD) == PM.words(seed, off, n // 4)).any()
    quads = [tuple(PM.words(7, o, 1)[0]) for o in (2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1)]
    assert len(set(quads)) == 3
    assert tuple(PM.words(7, 0, 1)[0]) not in quads and tuple(PM.words(7, 1, 1)[0]) not in quads  # the high counter word is not dropped
    # a stream that crosses 2^32 continues the one below it
    assert np.array_equal(PM.words(7, 2 ** 32 - 2, 4)[2:], PM.words(7, 2 ** 32, 2))
    for s in (0, 7, 2 ** 32 - 1):
        assert not (PM.words(s, 3, 4) == PM.words(s + 2 ** 32, 3, 4)).any()
    # modulo 2^64 in both arguments
    assert np.array_equal(PM.words(2 ** 64 + 7, 5, 2), PM.words(7, 5, 2))
    assert np.array_equal(PM.words(7, 2 ** 64 - 1, 3)[1:], PM.words(7, 0, 2))
    # element addressing: a stream at offset k is the tail of the stream at offset 0
    z, r = PM.randn_stream(7, 0, 45)
    z2, r2 = PM.randn_stream(7, 3, 33)
    assert np.array_equal(z[12:], z2) and np.array_equal(r[12:], r2)
    assert np.array_equal(PM.dropout_keep(7, 0, 45, 0.3)[12:], PM.dropout_keep(7, 3, 33, 0.3))


def test_dropout_keep_decision():
    w = PM.dropout_words(11, 5, 4096)
    top = (w >> np.uint32(8)).astype(np.int64)
    for p in (0.0, 0.1, 0.2, 0.5, 0.999):
        keep = PM.dropout_keep(11, 5, 4096, p)
        thr = float(np.float32(p)) * 2.0 ** 24
        assert np.array_equal(keep, top >= thr)
        assert abs(keep.mean() - (1 - p)) < 6 * np.sqrt(max(p * (1 - p), 1e-9) / 4096) + 1e-12
    assert PM.dropout_keep(11, 5, 4096, 0.0).all()
    j = int(np.argmax((top > 0) & (top < 2 ** 24 - 1)))
    assert PM.dropout_keep(11, 5, 4096, top[j] / 2.0 ** 24)[j]            # u == p: kept
    assert not PM.dropout_keep(11, 5, 4096, (top[j] + 1) / 2.0 ** 24)[j]  # the next p: dropped


@pytest.mark.parametrize("seed", PM.MOMENT_SEEDS)
def test_model_moments_meet_the_gpu_bounds(seed):
    z, r = PM.randn_stream(seed, 0, 1 << 20)
    mean, std, m4 = PM.moments(z)
    assert abs(mean) < 5e-3 and abs(std - 1.0) < 5e-3 and abs(m4 - 3.0) < 0.05, (mean, std, m4)
    assert np.abs(z).max() <= np.sqrt(48.0 * np.log(2.0)) and (r >= 0).all()


def test_the_sweep_lists_every_value():
    assert {s for _, s, _, _ in PM.STREAMS} >= set(PM.SEEDS)
    assert {o for _, _, o, _ in PM.STREAMS} >= set(PM.OFFSETS)
    assert {n for _, _, _, n in PM.STREAMS} >= set(PM.LENGTHS)
    assert max(n for _, _, _, n in PM.STREAMS) <= 2 ** 16 + 3
