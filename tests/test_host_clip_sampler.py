"""Device-side clip sampler, host side: the C-ABI entry and what it refuses before any launch, the resampling table, the quality of
the filter design through the float64 restatement (tests/clip_cases.py), and DeviceClipSampler.draw.

The quality figures belong to the filter (Z = 16, P = 256, beta 9, rolloff 0.945) and the restatement, not to the kernel.  Measured
on a CPU: sines of frequency f <= 0.33 c cycles/sample (c = min(1, 1/rate)) come back with max error 1.6e-5 to 1.8e-5 at rates
0.5, 0.8909, 1 + 2^-20, 1.1225 and 2; DC with 1.1e-5 to 1.7e-5; at rate 2 a tone at 0.3 or 0.4 cycles/sample (above the new
Nyquist) comes out at 2.3e-5 and 1.2e-5 relative rms.  Each is asserted at 5e-5, 2 - 4 x the measured value."""
import ctypes

import numpy as np
import pytest
import torch

import clip_cases as C

RATES = [0.5, 0.8909, 1 + 2.0 ** -20, 1.1225, 2.0]


def test_entry_declared_and_exported():
    from hifigan_modified import _native
    decl = _native.declared_symbols()
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert "mv_clip_gather" in decl and len(decl["mv_clip_gather"][1]) == 12
    assert hasattr(lib, "mv_clip_gather")


def _call(B=2, T=256, Z=16, P=256, src_kind=0, dtype=0, null=None):
    """mv_clip_gather with dummy non-null pointers: only for argument sets it refuses, which it does before any launch."""
    from hifigan_modified import _native
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    ptr = {n: (None if n == null else p) for n in ("arena", "descs", "table", "wave")}
    return _native.lib().mv_clip_gather(ptr["arena"], src_kind, ptr["descs"], ptr["table"], Z, P, ptr["wave"], B, T, 7, dtype, None)


@pytest.mark.parametrize("kw", [dict(B=0), dict(B=-3), dict(T=0), dict(T=(1 << 20) + 1), dict(Z=0), dict(Z=65), dict(P=0),
                                dict(P=1025), dict(src_kind=2), dict(src_kind=-1), dict(null="arena"), dict(null="descs"),
                                dict(null="table"), dict(null="wave")])
def test_entry_refuses_bad_arguments(kw):
    assert _call(**kw) == -1                                     # MV_ERR_ARG


def test_entry_refuses_unknown_dtype():
    assert _call(dtype=7) == -2                                  # MV_ERR_DTYPE
    assert _call(dtype=-1) == -2


def test_record_layout():
    from hifigan_modified.data import CLIP_DESC
    assert CLIP_DESC == C.DESC and C.DESC.itemsize == 48
    assert [C.DESC.fields[n][1] for n in C.DESC.names] == [0, 8, 16, 24, 32, 36, 40]


def test_table():
    import hifigan_modified as H
    t = H.resample_table()
    assert t.dtype == torch.float32 and t.shape == (16 * 256 + 1,) and t[0] == np.float32(0.945)
    t = H.resample_table(Z=3, P=7, beta=5.0, rolloff=0.9)
    assert t.shape == (22,) and t[0] == np.float32(0.9)
    z = np.arange(22) / 7.0
    want = 0.9 * np.sinc(0.9 * z) * np.i0(5.0 * np.sqrt(np.maximum(1 - (z / 3) ** 2, 0))) / np.i0(5.0)
    assert np.array_equal(t.numpy(), want.astype(np.float32))


@pytest.fixture(scope="module")
def table():
    import hifigan_modified as H
    return H.resample_table().numpy()


def _through(x, rate, table, T=256, pos=300.37):
    rec = C.records([(0, len(x), C.q32(pos), C.q32(rate), 1.0, 0.0, 0)])[0]
    s = C.resample(x.astype(np.float32), rec, table, 16, 256, T)
    at = (int(rec["pos_q32"]) + np.arange(T) * int(rec["rate_q32"])) / C.Q32     # the exact positions, in float64
    return s, at


@pytest.mark.parametrize("rate", RATES)
def test_restatement_reproduces_passband_sines_and_dc(rate, table):
    n, c = 1200, min(1.0, 1.0 / rate)
    j = np.arange(n)
    worst = 0.0
    for f in (0.013, 0.1 * c, 0.21 * c, 0.33 * c):
        x = np.sin(2 * np.pi * f * j + 0.4).astype(np.float32).astype(np.float64)      # the fp32 samples are the signal
        s, at = _through(x, rate, table)
        worst = max(worst, np.abs(s - np.sin(2 * np.pi * f * at + 0.4)).max())
    s, _ = _through(np.ones(n), rate, table)
    dc = np.abs(s - 1).max()
    print(f"rate {rate}: sines max error {worst:.2e}, DC error {dc:.2e}")
    assert worst <= 5e-5
    assert dc <= 5e-5


@pytest.mark.parametrize("f", [0.3, 0.4])
def test_restatement_rejects_tones_above_the_new_nyquist(f, table):
    x = np.sin(2 * np.pi * f * np.arange(1200) + 0.4)
    s, _ = _through(x, 2.0, table)
    rel = np.sqrt(np.mean(s ** 2)) / np.sqrt(np.mean(x ** 2))
    print(f"rate 2, tone {f}: relative rms {rel:.2e}")
    assert rel <= 5e-5


def test_fp32_emulation_is_close_to_the_restatement(table):
    """the emulation the GPU test takes its tolerance from: the same arithmetic, so it differs from float64 by rounding only."""
    x = np.random.default_rng(0).uniform(-1, 1, 700).astype(np.float32)
    for rate in RATES:
        rec = C.records([(0, 700, C.q32(20.3), C.q32(rate), 1.0, 0.0, 0)])[0]
        e = np.abs(C.resample(x, rec, table, 16, 256, 300, np.float32) - C.resample(x, rec, table, 16, 256, 300)).max()
        assert 0 < e < 1e-5, (rate, e)


def test_copy_records_in_the_restatement():
    x = np.arange(1, 11, dtype=np.float32)
    rec = C.records([(2, 5, C.q32(-2), C.Q32, 1.0, 0.0, 0)])[0]
    assert C.is_copy(rec)
    assert np.array_equal(C.resample(x, rec, np.zeros(5, np.float32), 2, 2, 9), [0, 0, 3, 4, 5, 6, 7, 0, 0])
    assert not C.is_copy(C.records([(0, 5, 1, C.Q32, 1.0, 0.0, 0)])[0])              # rate 1, fractional position
    pcm = np.array([-32768, 16384, 32767], dtype=np.int16)
    assert np.array_equal(C.decode(pcm), [-1.0, 0.5, 32767 / 32768])


def test_normals_restatement():
    z = C.normals(1 << 16, 5, 9)
    assert np.abs(z).max() <= 5.77 and abs(z.mean()) < 5 / 256 and abs(z.var() - 1) < 0.02
    assert np.array_equal(z[:1001], C.normals(1001, 5, 9))
    assert not np.array_equal(z[:64], C.normals(64, 5, 10)) and not np.array_equal(z[:64], C.normals(64, 6, 9))


# ------------------------------------------------------------------------------------------------------ DeviceClipSampler.draw
def _utts():
    g = torch.Generator().manual_seed(3)
    return [torch.rand(n, generator=g) * 2 - 1 for n in (5000, 300, 1000, 12000, 5)]


def _sampler(**kw):
    import hifigan_modified as H
    kw.setdefault("clip_samples", 1024)
    return H.DeviceClipSampler(_utts(), device="cpu", **kw)          # the arena lives wherever `device` says; draw() is host only


def test_draw_is_deterministic_per_seed_and_rank():
    import hifigan_modified as H
    aug = H.DeviceClipSampler.reference_augmentation()
    a, b = _sampler(seed=4, rank=1, **aug).draw(16), _sampler(seed=4, rank=1, **aug).draw(16)
    assert a.dtype == C.DESC and a.tobytes() == b.tobytes()
    other = _sampler(seed=4, rank=0, **aug).draw(16)
    assert other.tobytes() != a.tobytes()
    assert not np.array_equal(other["src_off"], a["src_off"]) or not np.array_equal(other["pos_q32"], a["pos_q32"])


def test_draw_without_augmentation_equals_clip_sampler():
    import hifigan_modified as H
    for seed, rank in ((0, 0), (7, 2)):
        ref = H.ClipSampler(_utts(), clip_samples=1024, seed=seed, rank=rank, device="cpu")
        s = _sampler(seed=seed, rank=rank)
        for _ in range(3):
            rec = s.draw(9)
            assert s.picks(rec) == ref.draw(9)
            assert all(C.is_copy(r) for r in rec) and (rec["gain"] == 1).all() and (rec["noise_std"] == 0).all()
    assert list(rec["noise_ctr"]) == list(range(18, 27))                 # a running clip counter


def test_draw_augmentation_ranges():
    import hifigan_modified as H
    aug = H.DeviceClipSampler.reference_augmentation()
    assert aug == dict(rate_range=(2 ** (-2 / 12), 2 ** (2 / 12)), noise_level=0.01)
    rec = _sampler(seed=1, gain_db_range=(-6.0, 3.0), **aug).draw(200)
    rate = rec["rate_q32"] / C.Q32
    assert rate.min() >= 2 ** (-2 / 12) - 1e-9 and rate.max() <= 2 ** (2 / 12) + 1e-9
    assert rate.min() < 0.92 and rate.max() > 1.09 and abs(np.log(rate).mean()) < 0.02      # log-uniform: the log is centred
    db = 20 * np.log10(rec["gain"])
    assert db.min() >= -6.0001 and db.max() <= 3.0001 and db.min() < -5 and db.max() > 2
    assert (rec["noise_std"] == np.float32(0.01)).all()
    assert list(rec["noise_ctr"]) == list(range(200))
    lens = {0: 5000, 5000: 300, 5300: 1000, 6300: 12000, 18300: 5}
    for r in rec:
        n, need = lens[int(r["src_off"])], -(-1024 * int(r["rate_q32"]) // C.Q32)
        assert int(r["src_len"]) == n and int(r["pos_q32"]) & 0xFFFFFFFF == 0
        assert 0 <= int(r["pos_q32"]) >> 32 <= max(n - need, 0)
    half = _sampler(seed=1, p_augment=0.5, **aug).draw(400)
    plain = np.array([C.is_copy(r) and r["noise_std"] == 0 for r in half])
    assert 150 < plain.sum() < 250                                       # about half are left alone


def test_need_and_start_bounds_at_rate_two():
    import hifigan_modified as H
    s = H.DeviceClipSampler([torch.zeros(1500), torch.zeros(2100)], clip_samples=1024, device="cpu", rate_range=(2.0, 2.0))
    rec = s.draw(64)
    assert (rec["rate_q32"] == 2 * C.Q32).all()
    starts = {0: set(), 1500: set()}
    for r in rec:
        starts[int(r["src_off"])].add(int(r["pos_q32"]) >> 32)
    assert starts[0] == {0}                                              # 1500 < need = 2048: only start 0, the tail is zero padding
    assert max(starts[1500]) <= 2100 - 2048 and len(starts[1500]) > 1


def test_state_dict_round_trip_continues_the_stream():
    import hifigan_modified as H
    aug = H.DeviceClipSampler.reference_augmentation()
    a = _sampler(seed=2, **aug)
    a.draw(5)
    sd = a.state_dict()
    nxt = a.draw(7)
    b = _sampler(seed=99, **aug)
    b.load_state_dict(sd)
    assert b.draw(7).tobytes() == nxt.tobytes()
    assert int(nxt["noise_ctr"][0]) == 5


def test_constructor_and_op_checks():
    import hifigan_modified as H
    from hifigan_modified import ops
    with pytest.raises(ValueError):
        H.DeviceClipSampler([], device="cpu")
    with pytest.raises(ValueError):
        _sampler(storage="int8")
    with pytest.raises(ValueError):
        _sampler(rate_range=(0.4, 1.0))
    s = _sampler(storage="pcm16")
    assert s.arena.dtype == torch.int16 and s.arena.numel() == 18305
    u = _utts()[0]
    assert torch.equal(s.arena[:5000], torch.clamp(torch.round(u * 32768), -32768, 32767).to(torch.int16))
    raw = H.DeviceClipSampler([torch.tensor([-32768, 5, 32767], dtype=torch.int16)], device="cpu", storage="pcm16")
    assert raw.arena.tolist() == [-32768, 5, 32767]
    descs = torch.zeros(2, 6, dtype=torch.int64)
    tab = H.resample_table()
    with pytest.raises(ValueError):
        ops.clip_gather(torch.zeros(10), descs, tab[:-1], 16, 256, 64, 0)            # table length
    with pytest.raises(ValueError):
        ops.clip_gather(torch.zeros(10), descs.view(-1)[:11], tab, 16, 256, 64, 0)   # not whole records
    with pytest.raises(ValueError):
        ops.clip_gather(torch.zeros(10, dtype=torch.float64), descs, tab, 16, 256, 64, 0)
    with pytest.raises(ValueError):
        ops.clip_gather(torch.zeros(10), descs, tab, 16, 256, 0, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.clip_gather(torch.zeros(10), descs, tab, 16, 256, 64, 0)
