"""Numpy models of the random streams of csrc/philox.h, written from the published generator and the header's comments, not from its code.

Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011; the Random123 library): a 128-bit
counter (c0, c1, c2, c3) and a 64-bit key (k0, k1).  One round:
    (hi0, lo0) = 0xD2511F53 * c0      (hi1, lo1) = 0xCD9E8D57 * c2        (32 x 32 -> 64 bit products)
    (c0, c1, c2, c3) <- (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0)
and between rounds the key is bumped by the Weyl constants (0x9E3779B9, 0xBB67AE85).  Ten rounds, nine bumps.

What the project draws from it (one counter value = four 32-bit words = four consecutive elements, "quad" q holds elements 4 q .. 4 q + 3):
  normals   counter (lo32(offset + q), hi32(offset + q), 0, 0), key (lo32(seed), hi32(seed)); word k -> u_k = ((w_k >> 8) + 1) / 2^24 in
            (0, 1]; Box-Muller: r0 = sqrt(-2 ln u0), theta0 = 2 pi u1, r1 = sqrt(-2 ln u2), theta1 = 2 pi u3;
            z = (r0 cos theta0, r0 sin theta0, r1 cos theta1, r1 sin theta1)
  dropout   counter (lo32(offset + q), hi32(offset + q), 0x5eed, 0), same key; element 4 q + k is kept iff (w_k >> 8) / 2^24 >= float32(p)
seed and offset + q are taken modulo 2^64.  Everything here is float64 / integer exact; the models never round to float32."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
MUL0, MUL1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
WEYL0, WEYL1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
DROPOUT_WORD = 0x5EED
MASK64 = (1 << 64) - 1


def _u64(v):
    return np.atleast_1d(np.asarray(v, dtype=np.uint64)) & M32


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Counter and key words as (arrays of) integers < 2^32 -> the four output words, uint32 arrays, in output order."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[_u64(v) for v in (c0, c1, c2, c3, k0, k1)])
    for rnd in range(10):
        if rnd:
            k0, k1 = (k0 + WEYL0) & M32, (k1 + WEYL1) & M32
        p0, p1 = MUL0 * c0, MUL1 * c2  # < 2^64: no wrap
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def words(seed, offset, n_quads, third=0):
    """[n_quads, 4] uint32: the words of quads 0 .. n_quads - 1 of the stream (seed, offset) with third counter word `third`."""
    seed, offset = int(seed) & MASK64, int(offset) & MASK64
    with np.errstate(over="ignore"):
        ctr = np.uint64(offset) + np.arange(n_quads, dtype=np.uint64)  # wraps modulo 2^64
    w = philox4x32_10(ctr & M32, ctr >> np.uint64(32), third, 0, seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(w, axis=1)


def uniforms(w):
    """(0, 1] uniforms of words: ((w >> 8) + 1) / 2^24, exact in float64 (and in float32)."""
    return ((w >> np.uint32(8)).astype(np.float64) + 1.0) / 16777216.0


def box_muller(w):
    """[Q, 4] words -> (z [Q, 4], r [Q, 4]) in float64; r[:, k] is the radius that scales element k."""
    u = uniforms(w)
    r0, r1 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    t0, t1 = 2.0 * np.pi * u[:, 1], 2.0 * np.pi * u[:, 3]
    z = np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1), r1 * np.sin(t1)], axis=1)
    return z, np.stack([r0, r0, r1, r1], axis=1)


def randn_stream(seed, offset, n):
    """The n normals set_randn(seed, offset) writes, in float64, and the Box-Muller radius of each."""
    z, r = box_muller(words(seed, offset, (n + 3) // 4))
    return z.reshape(-1)[:n], r.reshape(-1)[:n]


def dropout_words(seed, offset, n):
    """The word behind each of the n keep decisions of the dropout stream (seed, offset)."""
    return words(seed, offset, (n + 3) // 4, DROPOUT_WORD).reshape(-1)[:n]


def dropout_keep(seed, offset, n, p):
    """bool [n]: keep iff (w >> 8) >= float32(p) * 2^24 -- both sides exact in float64."""
    w = dropout_words(seed, offset, n)
    return (w >> np.uint32(8)).astype(np.float64) >= float(np.float32(p)) * 16777216.0


def normal_bound(z, r, k):
    """|fp32 Box-Muller - float64| allowed for a kernel that forms the angle as fl(fl32(2 pi) u) and whose logf, sqrtf, sincosf and final
    product together cost k fp32 ulp: u is exact; the angle is off by at most half an ulp of a number in [4, 8) (2^-22) plus
    |fl32(2 pi) - 2 pi| u <= 1.75e-7, together < 2^-21, which moves z by at most r times that; the rest is relative to the radius (the
    error of sin / cos is absolute in units of 1) or to the result."""
    return r * 2.0 ** -21 + k * 2.0 ** -24 * np.maximum(r, np.abs(z))


# Box-Muller extremes at seed 0 (found by a search over the first 2^26 counters; the tests evaluate only these): (quad counter, word, what)
EXTREMES = [
    (17758991, 0, "zero"),   # u0 = 2^-24: the largest radius
    (38471471, 0, "ones"),   # u0 = 1: r0 = 0
    (17169035, 1, "zero"),   # the smallest angle
    (44150062, 1, "ones"),   # u1 = 1: the angle is fl(2 pi)
    (21603008, 2, "zero"),
    (18082804, 2, "ones"),
    (40983361, 3, "zero"),
    (35204404, 3, "ones"),
]

# the seeds, offsets and lengths of the GPU sweep; (name, seed, offset, n).  Every listed value appears at least once.
SEEDS = [0, 7, 2 ** 32 - 1, 2 ** 32, 0xDEADBEEF12345678, 2 ** 64 - 1]
OFFSETS = [0, 5, 2 ** 32 - 2, 2 ** 32, 5 * 2 ** 28 + 3, 17 * 2 ** 28, 2 ** 63 + 1]
LENGTHS = [1, 2, 3, 4, 5, 1023, 1024, 1027, 2 ** 16 + 3]
STREAMS = [
    ("known_answer_quad", 0, 0, 4),
    ("carry_crossing", 7, 2 ** 32 - 2, 1027),              # quads 0, 1 below 2^32, quad 2 at 2^32: the carry inside the call
    ("both_high_words", 0xDEADBEEF12345678, 17 * 2 ** 28, 1023),
    ("seed_low_word_full", 2 ** 32 - 1, 5, 1),
    ("seed_high_word_only", 2 ** 32, 2 ** 32, 2),
    ("seed_all_ones", 2 ** 64 - 1, 2 ** 63 + 1, 3),
    ("site_offset", 7, 5 * 2 ** 28 + 3, 5),
    ("block_exact", 2 ** 32, 0, 1024),
    ("many_blocks_partial_quad", 0xDEADBEEF12345678, 2 ** 32 - 2, 2 ** 16 + 3),
    ("wrapping_counter", 7, 2 ** 64 - 1, 5),               # offset + q wraps modulo 2^64
]
MOMENT_SEEDS = [7, 8]  # test_posterior_qsample_randn


def moments(z):
    z = np.asarray(z, dtype=np.float64)
    return float(z.mean()), float(z.std(ddof=1)), float((z ** 4).mean())
