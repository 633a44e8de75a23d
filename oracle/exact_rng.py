"""The device random draws restated in numpy integer arithmetic: Philox-4x32-10, the uniform / Box-Muller maps and the Feistel pixel
permutation of csrc/dn_rng.h.

TEST INFRASTRUCTURE ONLY (see nerf_oracle.py header): the product never imports this module and this module imports nothing of the
product.  Written from the Philox paper (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11, section
3.3 and the Random123 constants) and from the words of dn_rng.h's comments; pinned to the Random123 known-answer vectors in
tests/test_device_draws.py.

Philox-4x32, one round on the counter (c0, c1, c2, c3) with the round key (k0, k1):
    (hi0, lo0) = 0xD2511F53 * c0        (hi1, lo1) = 0xCD9E8D57 * c2        (32 x 32 -> 64 bits)
    (c0, c1, c2, c3) <- (hi1 ^ c1 ^ k0,  lo1,  hi0 ^ c3 ^ k1,  lo0)
ten rounds, the key raised by the Weyl constants (0x9E3779B9, 0xBB67AE85) between rounds.

The layout of a draw:  key = (seed_lo, seed_hi),  counter = (index_lo, index_hi, stream, iteration).
Streams: 0 stratified jitter, 1 coarse density noise, 2 resampling u, 3 fine density noise, 4 pixel permutation, 5 training view.

Every array is uint64 holding 32-bit values; products of two 32-bit values fit 64 bits exactly."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
MUL_A = np.uint64(0xD2511F53)
MUL_B = np.uint64(0xCD9E8D57)
WEYL_A = 0x9E3779B9
WEYL_B = 0xBB67AE85
SHIFT32 = np.uint64(32)

STREAM_JITTER, STREAM_NOISE_COARSE, STREAM_U, STREAM_NOISE_FINE, STREAM_PIXELS, STREAM_VIEW = range(6)

TWO_PI_F32 = np.float32(6.283185307179586)
INV_2_24 = np.float32(1.0 / 16777216.0)


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def philox4x32_10(k0, k1, c0, c1, c2, c3):
    """Four output words (uint64 arrays of 32-bit values, broadcast over the arguments) of Philox-4x32-10."""
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    c0, c1, c2, c3 = np.broadcast_arrays(_u64(c0) & M32, _u64(c1) & M32, _u64(c2) & M32, _u64(c3) & M32)
    for _ in range(10):
        prod_a = MUL_A * c0
        prod_b = MUL_B * c2
        c0, c1, c2, c3 = ((prod_b >> SHIFT32) ^ c1 ^ np.uint64(k0), prod_b & M32, (prod_a >> SHIFT32) ^ c3 ^ np.uint64(k1), prod_a & M32)
        k0 = (k0 + WEYL_A) & 0xFFFFFFFF
        k1 = (k1 + WEYL_B) & 0xFFFFFFFF
    return c0, c1, c2, c3


def rng_words(seed, iteration, stream, index):
    """The four words of element `index` (integer or array, up to 64 bits) of `stream` in `iteration` under the 64-bit `seed`."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    index = _u64(index)
    return philox4x32_10(seed & 0xFFFFFFFF, seed >> 32, index & M32, index >> SHIFT32, int(stream) & 0xFFFFFFFF, int(iteration) & 0xFFFFFFFF)


def _to_uniform(word):
    """The top 24 bits of a word as fp32 in [0, 1): an integer below 2^24 times 2^-24, both exact in fp32."""
    return (word >> np.uint64(8)).astype(np.float32) * INV_2_24


def uniform(seed, iteration, stream, index):
    return _to_uniform(rng_words(seed, iteration, stream, index)[0])


def normal_f64(seed, iteration, stream, index):
    """(z, u1, u2): Box-Muller evaluated in float64 on the fp32 arguments the kernel forms - u1 = ((w0 >> 8) + 1) 2^-24 in (0, 1]
    (exact), u2 = (w1 >> 8) 2^-24 (exact), the angle float32(2 pi) * u2 rounded to fp32; z = sqrt(-2 ln u1) cos(angle)."""
    w0, w1, _, _ = rng_words(seed, iteration, stream, index)
    u1 = ((w0 >> np.uint64(8)) + np.uint64(1)).astype(np.float32) * INV_2_24
    u2 = _to_uniform(w1)
    angle = TWO_PI_F32 * u2
    assert u1.dtype == np.float32 and angle.dtype == np.float32
    z = np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(angle.astype(np.float64))
    return z, u1, u2


def feistel_bits(n):
    """The smallest even bit count, at least 2, whose domain 2^bits covers n."""
    bits = 2
    while (1 << bits) < n:
        bits += 2
    return bits


def feistel_permute(i, n, seed, iteration, want_passes=False):
    """perm(i) for a keyed permutation of [0, n): a balanced 4-round Feistel network on feistel_bits(n) bits, re-applied to a value
    until it falls below n (cycle walking).  Round `round` maps (l, r) to (r, l ^ F(r)), F(r) = the low half-width bits of word 0 of
    the generator on counter (r, round, 4, iteration)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    n = int(n)
    half = np.uint64(feistel_bits(n) // 2)
    mask = np.uint64((1 << int(half)) - 1)
    x = _u64(i).copy().reshape(-1)
    assert x.size == 0 or int(x.max()) < n
    todo = np.arange(x.size)
    passes = 0
    while todo.size:
        v = x[todo]
        left, right = v >> half, v & mask
        for rnd in range(4):
            f = philox4x32_10(k0, k1, right, rnd, STREAM_PIXELS, iteration)[0]
            left, right = right, left ^ (f & mask)
        v = (left << half) | right
        x[todo] = v
        todo = todo[v >= np.uint64(n)]
        passes += 1
    out = x.astype(np.int64).reshape(np.shape(i))
    return (out, passes) if want_passes else out


def drawn_view(seed, iteration, n_views):
    """The training view of an iteration: word 0 of element 0 of the view stream, modulo the number of views."""
    return int(rng_words(seed, iteration, STREAM_VIEW, 0)[0]) % int(n_views)
