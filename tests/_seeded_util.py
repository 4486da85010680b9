"""numpy restatement of the per-sample seeded noise (include/mdx.h: mdx_philox_u32 / mdx_randn_f32) -- the yardstick of
tests/test_seeded_noise_cpu.py and tests/test_seeded_noise_gpu.py.  It is written from the header's text, shares no code with
the library, and is itself pinned by the Random123 known answers (test_seeded_noise_cpu.py).

  words    Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (e >> 2, draw, stream, 0), element e <- word e & 3
  uniform  (2 (w >> 9) + 1) * 2^-24 in float64 (exact), rounded once to float32 (also exact)
  normal   Box-Muller in float64 on word pairs (0, 1), (2, 3): r = sqrt(-2 ln u_a); even element r cos(2 pi u_b), odd r sin
  dropout  keep where uniform(word under stream | 2^31) >= float32(p); kept values times float32(1) / (float32(1) - float32(p))
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
DROPOUT_BIT = 0x80000000

RNG_X_T, RNG_STEP, RNG_BLEND, RNG_ENCODE, RNG_POSTERIOR = 0, 1, 2, 3, 4


def philox4x32_10(counter, key):
    """counter: four uint64 arrays (or Python ints) holding 32-bit words, key: two.  Returns the four output words (uint64
    arrays holding 32-bit values).  Products of two 32-bit words fit uint64 exactly."""
    c = [np.asarray(x, dtype=np.uint64) for x in counter]
    k = [np.asarray(x, dtype=np.uint64) for x in key]
    m32, sh = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> sh) ^ c[1] ^ k[0], p1 & m32, (p0 >> sh) ^ c[3] ^ k[1], p0 & m32]
        k = [(k[0] + np.uint64(W0)) & m32, (k[1] + np.uint64(W1)) & m32]
    return c


def seed_pattern(seed):
    """A Python int in [-2^63, 2^64) as its 64-bit pattern."""
    seed = int(seed)
    assert -(1 << 63) <= seed < (1 << 64)
    return seed & ((1 << 64) - 1)


def words(seed, stream, draw, n):
    """[4, ceil(n / 4)] uint64: the output words of counters 0 .. ceil(n / 4) - 1 of one sample."""
    s = seed_pattern(seed)
    blk = np.arange((n + 3) // 4, dtype=np.uint64)
    z = np.zeros_like(blk)
    out = philox4x32_10((blk, z + np.uint64(draw), z + np.uint64(stream), z), (z + np.uint64(s & MASK32), z + np.uint64(s >> 32)))
    return np.stack(out)


def philox_u32(seed, stream, draw, n):
    """[n] uint32: element e = word e & 3 of counter e >> 2."""
    return words(seed, stream, draw, n).T.reshape(-1)[:n].astype(np.uint32)


def uniform(w):
    """float64 (2 (w >> 9) + 1) * 2^-24; exact, and unchanged by the rounding to float32 that follows."""
    u = (2.0 * (np.asarray(w, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 1.0) * 2.0 ** -24
    u32 = u.astype(np.float32)
    assert np.array_equal(u32.astype(np.float64), u)
    return u32


def normals64(seed, stream, draw, n):
    """[n] float64 N(0, 1): the Box-Muller restatement, unrounded."""
    w = words(seed, stream, draw, n)
    z = np.empty((w.shape[1], 4), dtype=np.float64)
    for pair in (0, 1):
        ua = uniform(w[2 * pair]).astype(np.float64)
        ub = uniform(w[2 * pair + 1]).astype(np.float64)
        r = np.sqrt(-2.0 * np.log(ua))
        z[:, 2 * pair] = r * np.cos(2.0 * np.pi * ub)
        z[:, 2 * pair + 1] = r * np.sin(2.0 * np.pi * ub)
    return z.reshape(-1)[:n]


def keep_mask(seed, stream, draw, n, p):
    """[n] bool: the dropout rule's kept elements."""
    return uniform(philox_u32(seed, stream | DROPOUT_BIT, draw, n)) >= np.float32(p)


def randn(seeds, stream, draw, n, scale=1.0, dropout=0.0):
    """[B, n] float64 restatement of mdx_randn_f32 (scale and 1 / (1 - p) as the float32 values the kernel is handed)."""
    rows = []
    for s in seeds:
        z = np.float64(np.float32(scale)) * normals64(s, stream, draw, n)
        if dropout > 0.0:
            inv = np.float64(np.float32(1.0) / (np.float32(1.0) - np.float32(dropout)))
            z = np.where(keep_mask(s, stream, draw, n, dropout), z * inv, 0.0)
        rows.append(z)
    return np.stack(rows)
