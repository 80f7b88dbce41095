"""The clip sampler's arithmetic (mv_clip_gather, include/mi355x_vocoder.h) restated in numpy, for the host and the GPU tests.

  resample(..., np.float64)  the definition: exact Q32.32 positions, every product and sum in float64, from the same fp32 table and
                             the same records the kernel gets.
  resample(..., np.float32)  the kernel's arithmetic operation by operation in fp32 (fr and c rounded as the kernel rounds them, the
                             taps summed in ascending j, no FMA): what fp32 costs against the definition.  The GPU test takes its
                             tolerance from this, recomputed on its own inputs.
  normals                    Philox4x32-10 + Box-Muller as the header defines them, in float64.
No GPU, no package import: the record layout is restated here as well."""
import numpy as np

Q32 = 1 << 32
DESC = np.dtype([("src_off", "<i8"), ("src_len", "<i8"), ("pos_q32", "<i8"), ("rate_q32", "<i8"),
                 ("gain", "<f4"), ("noise_std", "<f4"), ("noise_ctr", "<i8")])
_M32 = np.uint64(0xFFFFFFFF)


def records(rows):
    """[(src_off, src_len, pos_q32, rate_q32, gain, noise_std, noise_ctr)] -> structured array of 48-byte records."""
    rec = np.zeros(len(rows), dtype=DESC)
    for r, row in enumerate(rows):
        rec[r] = tuple(row)
    return rec


def q32(x):
    """a real position or rate as Q32.32 (rounded to nearest)."""
    return int(round(x * Q32))


def decode(arena):
    """the arena as float64 samples (16-bit PCM decodes as q * 2^-15)."""
    a = np.asarray(arena)
    return a.astype(np.float64) * 2.0 ** -15 if a.dtype == np.int16 else a.astype(np.float64)


def is_copy(rec):
    rate = min(max(int(rec["rate_q32"]), Q32 // 2), 2 * Q32)
    return rate == Q32 and int(rec["pos_q32"]) & 0xFFFFFFFF == 0


def _fetch(x, off, n, j):
    """x[j] of the utterance at (off, n), zero outside it."""
    ok = (j >= 0) & (j < n)
    return np.where(ok, x[off + np.where(ok, j, 0)], 0.0)


def resample(arena, rec, table, Z, P, T, ft=np.float64):
    """s[t] for one record (before gain and noise), all arithmetic in `ft`; the positions are exact integers either way."""
    x = decode(arena).astype(ft)
    off, n = int(rec["src_off"]), int(rec["src_len"])
    rate = min(max(int(rec["rate_q32"]), Q32 // 2), 2 * Q32)
    q = np.int64(int(rec["pos_q32"])) + np.arange(T, dtype=np.int64) * np.int64(rate)
    i = q >> np.int64(32)
    if is_copy(rec):
        return _fetch(x, off, n, i).astype(ft)
    lo = (q & np.int64(0xFFFFFFFF)).astype(np.uint32)
    tab = np.asarray(table, dtype=np.float32).astype(ft)
    if ft is np.float32:
        fr = lo.astype(np.float32) * np.float32(2.0 ** -32)
        c = min(np.float32(1), np.float32(2.0 ** 32) / np.float32(rate))
    else:
        fr = lo.astype(np.float64) * 2.0 ** -32
        c = min(1.0, Q32 / rate)
    c, Zf, Pf = ft(c), ft(Z), ft(P)
    W = (Z * max(rate, Q32) + Q32 - 1) >> 32            # ceil(Z / c): no tap outside i - W .. i + W + 1 can be within Z / c
    acc = np.zeros(T, dtype=ft)
    for m in range(-W, W + 2):                          # ascending j, the kernel's order
        a = np.abs(ft(m) - fr) * c
        u = a * Pf
        k = np.minimum(u.astype(np.int64), Z * P - 1)
        w = u - k.astype(ft)
        h = tab[k] + w * (tab[k + 1] - tab[k])
        acc = acc + np.where(a <= Zf, _fetch(x, off, n, i + m) * h, ft(0))
    assert acc.dtype == ft
    return c * acc


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on uint64 arrays holding 32-bit words -> four arrays of words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0) & _M32, np.uint64(k1) & _M32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def normals(T, key, ctr):
    """z[0..T) of the stream (key, ctr), float64: counter (t/4 lo, t/4 hi, ctr lo, ctr hi); words (r0, r1) give elements 4k and
    4k+1, (r2, r3) elements 4k+2 and 4k+3."""
    key, ctr = key & 0xFFFFFFFFFFFFFFFF, ctr & 0xFFFFFFFFFFFFFFFF
    nblk = (T + 3) // 4
    blk = np.arange(nblk, dtype=np.uint64)
    r = philox(blk & _M32, blk >> np.uint64(32), np.full(nblk, ctr & 0xFFFFFFFF, np.uint64), np.full(nblk, ctr >> 32, np.uint64),
               key & 0xFFFFFFFF, key >> 32)
    z = np.empty((nblk, 4))
    for h in range(2):
        u1 = ((r[2 * h] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24       # (0, 1]
        u2 = (r[2 * h + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24                    # [0, 1)
        R = np.sqrt(-2.0 * np.log(u1))
        z[:, 2 * h] = R * np.cos(2 * np.pi * u2)
        z[:, 2 * h + 1] = R * np.sin(2 * np.pi * u2)
    return z.reshape(-1)[:T]


def expected(arena, recs, table, Z, P, T, key, ft=np.float64):
    """y [B, T] float64 = gain * s + noise_std * z for every record (gain and noise_std are the records' fp32 values)."""
    out = np.empty((len(recs), T))
    for b, rec in enumerate(recs):
        y = np.float64(rec["gain"]) * resample(arena, rec, table, Z, P, T, ft).astype(np.float64)
        if rec["noise_std"] != 0:
            y = y + np.float64(rec["noise_std"]) * normals(T, key, int(rec["noise_ctr"]))
        out[b] = y
    return out
