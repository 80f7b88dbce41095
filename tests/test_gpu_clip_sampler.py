"""Device-side clip sampler on the GPU: mv_clip_gather against slicing (copy path, bit exact), against the float64 restatement of
tests/clip_cases.py (resampling path, gain, noise), and DeviceClipSampler against ClipSampler and against itself.

Shapes: utterances of 5, 300, 1000 and 5000 samples back to back in one arena; T in {64, 1500, 4099} and B in {1, 5, 33}: a clip
smaller than a tile, ragged tiles, several tiles, rows whose start is not 16-byte aligned (T = 4099), for any power-of-two tile up to
4096.

Tolerances.
  resampling  4 x E32, E32 being the largest difference between the fp32 numpy emulation of the kernel's arithmetic
              (clip_cases.resample with np.float32) and the float64 restatement ON THE TEST'S OWN INPUTS (white noise, |x| <= 1);
              the factor covers the device's summation with FMA contraction.  E32 measured on a CPU on these inputs at Z = 16,
              P = 256 over the five rates: 3.4e-7 to 6.0e-7 per batch from rounding alone, and 1.9e-6 to 6.6e-6 in the batches
              where fp32 puts one tap on the other side of the window's edge |j - (i + fr)| c = Z than float64 does (the
              Kaiser window ends at table[-1] = -6.7e-6, not at 0; the kernel forms that distance with the emulation's
              operations, so it decides as the emulation does).  bf16 / fp16 outputs: half an ulp of the output type on top.
  noise       4e-6 per unit noise_std against the float64 Box-Muller of the same Philox words: |z| <= 5.77 (u1 >= 2^-24), and
              logf, sqrtf, cospif, sinpif within 1-2 ulp each put the error near 1.4e-6.
  everything else is bit exact."""
import numpy as np
import pytest
import torch

import clip_cases as C

pytestmark = pytest.mark.gpu

LENS = (5, 300, 1000, 5000)
OFFS = (0, 5, 305, 1305)
RATES = [0.5, 0.8909, 1 + 2.0 ** -20, 1.1225, 2.0]
TORCH_DT = [torch.float32, torch.bfloat16, torch.float16]
ROUND2 = 2 * 2.0 ** -24        # y = gain * s + noise_std * z with both terms present: the product gain * s and the sum round once each


@pytest.fixture(scope="module")
def H():
    import hifigan_modified as H
    from hifigan_modified import _native
    _native.lib()
    return H


@pytest.fixture(scope="module")
def corpus(H):
    """white noise in [-1, 1]: the fp32 arena, its 16-bit PCM form, both also on the device, and the default table."""
    x = np.random.default_rng(11).uniform(-1, 1, sum(LENS)).astype(np.float32)
    pcm = np.clip(np.round(x.astype(np.float64) * 32768), -32768, 32767).astype(np.int16)
    tab = H.resample_table()
    return {"fp32": x, "pcm16": pcm, "fp32_dev": torch.from_numpy(x).cuda(), "pcm16_dev": torch.from_numpy(pcm).cuda(),
            "table": tab.numpy(), "table_dev": tab.cuda()}


def gather(corpus, kind, rec, T, key=0, dtype=torch.float32, table=None, Z=16, P=256):
    from hifigan_modified import ops
    descs = torch.from_numpy(rec.view(np.int64).reshape(len(rec), 6)).cuda()
    tab = corpus["table_dev"] if table is None else table
    y = ops.clip_gather(corpus[kind + "_dev"], descs, tab, Z, P, T, key, dtype)
    assert y.shape == (len(rec), 1, T) and y.dtype == dtype
    return y.cpu()[:, 0]


def half_ulp(y, dtype):
    """half an ulp of `dtype` at |y| (float64 array): 2^(e - mantissa bits - 1), e the exponent of y, floored at the type's subnormals."""
    bits, emin = {torch.float32: (23, -126), torch.bfloat16: (7, -126), torch.float16: (10, -14)}[dtype]
    e = np.maximum(np.frexp(np.abs(y))[1] - 1, emin)
    return np.ldexp(0.5, e - bits)


# ------------------------------------------------------------------------------------------------------------- copy path
def copy_records(B, T):
    """starts at 0, before the start (negative position), running past the end, wholly outside, in utterances shorter than T."""
    rows = []
    for b in range(B):
        u = b % 4
        n = LENS[u]
        pos = [0, -17, n - 10, max(n - T, 0), n + 5, -T - 3, n // 2, -1][(b // 4 + b) % 8]
        rows.append((OFFS[u], n, pos << 32, C.Q32, 1.0, 0.0, b))
    return C.records(rows)


def sliced(x, rec, T):
    out = np.zeros((len(rec), T), dtype=np.float32)
    for b, r in enumerate(rec):
        off, n, s = int(r["src_off"]), int(r["src_len"]), int(r["pos_q32"]) >> 32
        lo, hi = max(s, 0), min(s + T, n)
        if hi > lo:
            out[b, lo - s:hi - s] = x[off + lo:off + hi]
    return out


@pytest.mark.parametrize("kind", ["fp32", "pcm16"])
@pytest.mark.parametrize("T", [64, 1500, 4099])
@pytest.mark.parametrize("B", [1, 5, 33])
def test_copy_path_is_bit_exact_against_slicing(corpus, kind, T, B):
    rec = copy_records(B, T)
    x = corpus[kind] if kind == "fp32" else (corpus[kind].astype(np.float32) * np.float32(2.0 ** -15))
    want = torch.from_numpy(sliced(x, rec, T))
    assert want.abs().max() > 0
    for dtype in TORCH_DT:
        got = gather(corpus, kind, rec, T, dtype=dtype)
        assert torch.equal(got, want.to(dtype)), (kind, T, B, dtype)


def test_sampler_without_augmentation_equals_clip_sampler(H, corpus):
    utts = [torch.from_numpy(corpus["fp32"][o:o + n]) for o, n in zip(OFFS, LENS)]
    fe = H.MelFrontEnd()
    ref = H.ClipSampler(utts, 2048, fe, seed=5, rank=1)
    dev = H.DeviceClipSampler(utts, 2048, fe, seed=5, rank=1)
    for _ in range(3):
        w0, m0 = ref.sample(5)
        w1, m1 = dev.sample(5)
        assert w1.shape == (5, 1, 2048) and w1.dtype == torch.float32 and w0.abs().max() > 0
        assert torch.equal(w0, w1) and torch.equal(m0, m1)


# ------------------------------------------------------------------------------------------------------- resampling path
def resample_records(B, T, rate):
    """fractional positions: within Z / c of both utterance ends (and beyond them), in the interior, in utterances shorter than
    the clip; every seventh record has rate 1 with a fractional position (filter path), every fifth is a copy record."""
    rq, reach = C.q32(rate), 16 * max(1.0, rate)
    rows = []
    for b in range(B):
        u = (b + 3) % 4
        n = LENS[u]
        pos = [-reach + 0.37, n - T * rate - reach / 2 + 0.81, n / 3 + 0.5, -0.25, n - reach + 0.13, 7 + 2.0 ** -31, n + reach - 1.5,
               -reach - 3.2][(b // 4 + b) % 8]
        if b % 7 == 6:
            rows.append((OFFS[u], n, C.q32(pos) | 1, C.Q32, 1.0, 0.0, b))
        elif b % 5 == 4:
            rows.append((OFFS[u], n, C.q32(np.floor(pos)), C.Q32, 1.0, 0.0, b))
        else:
            rows.append((OFFS[u], n, C.q32(pos), rq, 1.0, 0.0, b))
    return C.records(rows)


def check_resampled(corpus, kind, rec, T, table_np=None, table_dev=None, Z=16, P=256, dtypes=TORCH_DT):
    tab = corpus["table"] if table_np is None else table_np
    want = C.expected(corpus[kind], rec, tab, Z, P, T, 0)
    e32 = np.abs(C.expected(corpus[kind], rec, tab, Z, P, T, 0, np.float32) - want).max()
    # an emulation that is exact, or far off, measures nothing: rounding, plus at most a tap at the window's edge taken in or left out
    assert 0 < e32 < 1e-5 + abs(float(tab[-1]))
    for dtype in dtypes:
        got = gather(corpus, kind, rec, T, dtype=dtype, table=table_dev, Z=Z, P=P).double().numpy()
        tol = 4 * e32 + (half_ulp(want, dtype) if dtype != torch.float32 else 0.0)
        err = np.abs(got - want)
        print(f"{kind} T {T} B {len(rec)} {dtype}: E32 {e32:.2e}, max error {err.max():.2e}, worst error / tolerance {(err / tol).max():.2f}")
        assert (err <= tol).all(), (kind, T, dtype, err.max(), e32)
        copy = np.array([C.is_copy(r) for r in rec])
        if copy.any():                           # copy records of a mixed batch stay bit exact
            assert torch.equal(torch.from_numpy(got[copy]).to(dtype), torch.from_numpy(want[copy]).to(dtype))
    return want


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("T,B", [(64, 33), (1500, 5), (4099, 1), (4099, 5)])
def test_resampling_against_float64_restatement(corpus, rate, T, B):
    rec = resample_records(B, T, rate)
    assert not C.is_copy(rec[0]) and (B < 7 or not C.is_copy(rec[6]))
    want = check_resampled(corpus, "fp32", rec, T)
    assert np.abs(want).max() > 0.1


@pytest.mark.parametrize("rate", [0.8909, 2.0])
def test_resampling_from_pcm16(corpus, rate):
    check_resampled(corpus, "pcm16", resample_records(33, 1500, rate), 1500, dtypes=[torch.float32, torch.bfloat16])


@pytest.mark.parametrize("Z,P", [(64, 256), (3, 7), (1, 1), (64, 1024)])
def test_other_tables(H, corpus, Z, P):
    """(64, 256) and (64, 1024) are longer than the kernel keeps in LDS and are read from global memory; Z = 64 at rate 2 is the
    widest source span a tile can have."""
    tab = H.resample_table(Z, P)
    for rate in (2.0, 0.7):
        check_resampled(corpus, "fp32", resample_records(5, 1500, rate), 1500, tab.numpy(), tab.cuda(), Z, P, dtypes=[torch.float32])


def test_fraction_that_rounds_to_one(corpus):
    """low position bits of 2^32 - 2 become fr = 1.0 in fp32 at every output (rate 2 and 1 keep them): the tap at i + W + 1 then sits at
    a distance of exactly Z / c and is weighed with the table's last entry, where the exact position leaves it out.  The emulation
    rounds the same way, so this is part of E32 here (larger than elsewhere, about c * table[-1] = 3e-6)."""
    rows = [(OFFS[3], LENS[3], (50 << 32) - 2, r, 1.0, 0.0, 0) for r in (2 * C.Q32, C.Q32)]
    check_resampled(corpus, "fp32", C.records(rows), 1500, dtypes=[torch.float32])


def test_rate_is_clamped(corpus):
    rows = [(OFFS[3], LENS[3], C.q32(40.3), r, 1.0, 0.0, 0) for r in (C.Q32 // 4, C.Q32 // 2, 3 * C.Q32, 2 * C.Q32, 0, -C.Q32)]
    got = gather(corpus, "fp32", C.records(rows), 700)
    assert torch.equal(got[0], got[1]) and torch.equal(got[2], got[3]) and torch.equal(got[4], got[1]) and torch.equal(got[5], got[1])


# -------------------------------------------------------------------------------------------------------- gain and noise
def test_gain_without_noise_is_one_exact_product(corpus):
    T, g = 1500, np.float32(0.37)
    base = resample_records(5, T, 1.1225)
    rec = np.concatenate([base, base])
    rec["gain"][5:] = g
    got = gather(corpus, "fp32", rec, T).numpy()
    assert np.array_equal(got[5:], g * got[:5]) and np.abs(got[:5]).max() > 0.1


def noise_records(B, std, ctr0=100):
    return C.records([(OFFS[3], LENS[3], 0, C.Q32, 0.0, std, ctr0 + b) for b in range(B)])       # gain 0: y = noise_std * z


@pytest.mark.parametrize("T,B", [(64, 5), (1500, 33), (4099, 5)])
@pytest.mark.parametrize("std", [1.0, 0.01])
def test_noise_against_numpy_restatement(corpus, T, B, std):
    key = 0x1234567_89ABCDEF
    rec = noise_records(B, std, ctr0=(1 << 32) - 2)           # the counters cross into the high word
    want = C.expected(corpus["fp32"], rec, corpus["table"], 16, 256, T, key)
    got = gather(corpus, "fp32", rec, T, key=key).double().numpy()
    err = np.abs(got - want).max()
    print(f"noise T {T} B {B} std {std}: max error {err:.2e} ({err / np.float32(std):.2e} per unit)")
    assert err <= 4e-6 * np.float64(np.float32(std))
    assert np.abs(want).max() > 2 * std


def test_noise_on_top_of_a_resampled_clip(corpus):
    T, key = 1500, 77
    rec = resample_records(5, T, 0.8909)
    rec["gain"], rec["noise_std"] = np.float32(0.8), np.float32(0.01)
    want = C.expected(corpus["fp32"], rec, corpus["table"], 16, 256, T, key)
    plain = rec.copy()
    plain["noise_std"] = 0
    e32 = np.abs(C.expected(corpus["fp32"], plain, corpus["table"], 16, 256, T, key, np.float32)
                 - C.expected(corpus["fp32"], plain, corpus["table"], 16, 256, T, key)).max()
    got = gather(corpus, "fp32", rec, T, key=key).double().numpy()
    assert np.abs(got - want).max() <= 4 * e32 + 4e-6 * 0.01 + ROUND2 * np.abs(want).max()
    assert np.abs(got - C.expected(corpus["fp32"], plain, corpus["table"], 16, 256, T, key)).max() > 0.02


def test_noise_streams(corpus):
    T = 1500
    one = noise_records(1, 1.0, ctr0=9)
    a = gather(corpus, "fp32", one, T, key=3)
    assert torch.equal(a, gather(corpus, "fp32", one, T, key=3))                         # two launches, the same bits
    many = noise_records(5, 1.0, ctr0=6)                                                 # ctr 9 is row 3 here
    m = gather(corpus, "fp32", many, T, key=3)
    assert torch.equal(m[3], a[0])
    assert len({m[b].numpy().tobytes() for b in range(5)}) == 5                          # another ctr, another stream
    assert not torch.equal(gather(corpus, "fp32", one, T, key=4), a)                     # another key as well
    assert torch.equal(gather(corpus, "fp32", one, 64, key=3)[0], a[0, :64])             # and no dependence on T


def test_noise_moments(corpus):
    n = 1 << 18
    z = gather(corpus, "fp32", noise_records(1, 1.0), n, key=1).double().numpy()[0]
    print(f"noise over 2^18 samples: mean {z.mean():.2e}, var {z.var():.5f}, max |z| {np.abs(z).max():.3f}")
    assert abs(z.mean()) < 5 / np.sqrt(n) and abs(z.var() - 1) < 0.02 and np.abs(z).max() <= 5.78


# --------------------------------------------------------------------------------------------------------- sampler level
def _utts(corpus):
    return [torch.from_numpy(corpus["fp32"][o:o + n]) for o, n in zip(OFFS, LENS)]


@pytest.mark.parametrize("storage,dtype", [("fp32", torch.float32), ("pcm16", torch.bfloat16)])
def test_sampler_with_reference_preset(H, corpus, storage, dtype):
    fe = H.MelFrontEnd()
    kw = dict(clip_samples=2048, front_end=fe, seed=3, dtype=dtype, storage=storage, gain_db_range=(-6.0, 0.0),
              **H.DeviceClipSampler.reference_augmentation())
    a, b, c = (H.DeviceClipSampler(_utts(corpus), rank=r, **kw) for r in (0, 0, 1))
    wa, ma = a.sample(5)
    wb, mb = b.sample(5)
    wc, _ = c.sample(5)
    assert wa.shape == (5, 1, 2048) and wa.dtype == dtype and ma.shape == (5, 80, 8) and ma.dtype == torch.float32
    assert torch.isfinite(wa.float()).all() and torch.isfinite(ma).all() and wa.float().abs().max() > 0.05
    assert torch.equal(ma, fe(wa))
    assert torch.equal(wa, wb) and torch.equal(ma, mb) and not torch.equal(wa, wc)
    sd = a.state_dict()
    w2, m2 = a.sample(5)
    assert not torch.equal(w2, wa)
    r = H.DeviceClipSampler(_utts(corpus), rank=0, **{**kw, "seed": 3})
    r.load_state_dict(sd)
    w3, m3 = r.sample(5)
    assert torch.equal(w2, w3) and torch.equal(m2, m3)


def test_sampler_batch_against_restatement(H, corpus):
    """the sampler's own records, arena and key through the restatement: storage, table and key reach the kernel as drawn."""
    s = H.DeviceClipSampler(_utts(corpus), 1500, None, seed=8, rank=2, storage="pcm16", gain_db_range=(-3.0, 3.0), p_augment=0.7,
                            **H.DeviceClipSampler.reference_augmentation())
    assert s.key == 10 and np.array_equal(s.arena.cpu().numpy(), corpus["pcm16"])
    rec = s.draw(33)
    assert 0 < sum(C.is_copy(r) for r in rec) < 33
    got = s.gather(rec)[:, 0].double().cpu().numpy()
    plain = rec.copy()
    plain["noise_std"] = 0
    f64 = C.expected(corpus["pcm16"], plain, corpus["table"], 16, 256, 1500, 10)
    e32 = np.abs(C.expected(corpus["pcm16"], plain, corpus["table"], 16, 256, 1500, 10, np.float32) - f64).max()
    want = C.expected(corpus["pcm16"], rec, corpus["table"], 16, 256, 1500, 10)
    assert np.abs(got - want).max() <= 4 * e32 + 4e-6 * 0.01 + ROUND2 * np.abs(want).max()
