"""Split-operand fp32 discriminator stacks (set_fp32_operands("split")): fp32 storage on the channels-last MFMA kernels with every
operand split into hi + lo bf16 and three products per MAC (csrc/disc_fused.hip, Mma<float>).  Kernel entries and whole stacks
against fp64, split against exact at the training shape, the exact default left alone, training trajectories, the captured step,
re-packing after an optimizer step and the registered operator."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from oracle import vocoder_oracle as O

pytestmark = pytest.mark.gpu

CFG = dict(hidden_channels=64, upsample_factors=[4, 2])
HOP = 8


@pytest.fixture(scope="module")
def H():
    import hifigan_modified as H
    from hifigan_modified import _native
    _native.lib()
    return H


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ----------------------------------------------------------------------------------------------- kernel entries
@pytest.mark.parametrize("kh,kw,cin,cout,Hh,W", [(3, 3, 64, 128, 3, 200), (1, 15, 128, 64, 1, 300), (3, 3, 256, 32, 5, 130)])
def test_fp32_conv_and_wgrad_entries_vs_fp64(H, kh, kw, cin, cout, Hh, W):
    """mv_dconv_cl_fwd and mv_dconv_wgrad_cl with MV_F32 (split operands) return MV_OK and match fp64."""
    from hifigan_modified import _native as N, ops
    torch.manual_seed(0)
    B = 2
    w = torch.randn(cout, cin, kh, kw) / (cin * kh * kw) ** 0.5
    b = torch.randn(cout) * 0.1
    x = torch.randn(B, Hh, W, cin)
    g = torch.randn(B, Hh, W, cout)
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=(kh // 2, kw // 2)).permute(0, 2, 3, 1)
    xc, wc, bc = x.cuda().contiguous(), w.cuda().contiguous(), b.cuda()
    packed = ops.dconv_pack(wc, torch.float32, 0)
    y = torch.empty(B, Hh, W, cout, device="cuda")
    rc = N.lib().mv_dconv_cl_fwd(_p(xc), _p(packed), _p(bc), None, _p(y), B, Hh, W, cin, cout, kh, kw, 1, N.ACT_NONE, 0.1, N.MV_F32,
                                 ops._stream())
    assert rc == 0, rc
    e_fwd = O.rel_l2(y.cpu().double(), ref)
    gref = torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2), w.shape, g.double().permute(0, 3, 1, 2), padding=(kh // 2, kw // 2))
    gc = g.cuda().contiguous()
    ws = torch.empty(cout * cin * kh * kw + cout, device="cuda")
    gw = torch.empty(cout, cin, kh, kw, device="cuda")
    gb = ws[cout * cin * kh * kw:]
    rc = N.lib().mv_dconv_wgrad_cl(_p(xc), _p(gc), _p(gw), _p(gb), _p(ws), B, Hh, W, cin, cout, kh, kw, 1, N.MV_F32, ops._stream())
    assert rc == 0, rc
    e_gw = O.rel_l2(gw.cpu().double(), gref)
    e_gb = O.rel_l2(gb.cpu().double(), g.double().sum((0, 1, 2)))
    print(f"[split] entries {kh}x{kw} {cin}->{cout}: fwd {e_fwd:.1e} gw {e_gw:.1e} gb {e_gb:.1e}")
    assert e_fwd < 1.5e-5 and e_gw < 1.5e-5 and e_gb < 1.5e-5, (e_fwd, e_gw, e_gb)     # measured 2-5e-6


# ----------------------------------------------------------------------------------------------- whole stacks vs fp64
@pytest.mark.parametrize("kind,arg,T", [("2d", 2, 512), ("2d", 3, 1000), ("2d", 11, 700), ("1d", 1, 640), ("1d", 2, 1000), ("1d", 4, 1001)])
@pytest.mark.parametrize("slope", [1.0, 0.1])
def test_split_stack_vs_fp64(H, kind, arg, T, slope):
    """Forward, input gradient and all 10 parameter gradients of a split-mode stack against an fp64 CPU evaluation.
    slope 1.0 (linear stack: only rounding remains, the kernel-correctness bound): measured forward <= 1.2e-5, gradients <= 4.1e-5.
    slope 0.1: the forward stays at ~1e-5, but a pre-activation within ~1e-5 of zero takes the other LeakyReLU slope in one of the
    two evaluations, and each such flip moves every upstream gradient by ~1e-3 (rel-L2).  A few of the ~1e6 pre-activations flip,
    so the gradients are measured at 0-6e-3, set by the number of flips; the 2e-2 bound is that noise, not a kernel tolerance."""
    from hifigan_modified import disc_fused, functional as Fn
    torch.manual_seed(0)
    m = H.Discriminator2D(arg) if kind == "2d" else H.Discriminator1D(arg)
    torch.manual_seed(1)
    x32 = torch.randn(3, 1, T).clamp(-1, 1)
    ps = {k: v.detach().double().requires_grad_(True) for k, v in m.named_parameters()}
    xr = x32.double().requires_grad_(True)
    if kind == "2d":
        h = O.mpd_fold(xr, arg)
        for li, idx in enumerate((0, 2, 4, 6, 8)):
            h = F.conv2d(h, ps[f"conv_layers.{idx}.weight"], ps[f"conv_layers.{idx}.bias"], padding=1)
            if li < 4:
                h = torch.where(h >= 0, h, h * slope)
    else:
        h = xr[:, :, :T // arg * arg].reshape(3, 1, T // arg, arg).mean(3) if arg > 1 else xr
        for li, idx in enumerate((0, 2, 4, 6, 8)):
            h = F.conv1d(h, ps[f"conv_layers.{idx}.weight"], ps[f"conv_layers.{idx}.bias"], padding=7)
            if li < 4:
                h = torch.where(h >= 0, h, h * slope)
    torch.manual_seed(2)
    r = torch.randn_like(h)
    (h * r).sum().backward()
    m = m.cuda().set_fp32_operands("split")
    x = x32.cuda().requires_grad_(True)
    if slope == 0.1:
        y = m(x)                                     # the module's own route: functional.disc2d / disc1d -> the split stack
    else:
        x0 = (Fn._MpdFold.apply(x, arg) if T % arg else x.view(3, 1, arg, T // arg)) if kind == "2d" else \
            (Fn._AvgPool.apply(x, arg) if arg > 1 else x)
        y = disc_fused.disc_stack(x0, m, slope=slope)
    assert y.shape == h.shape and y.dtype == torch.float32
    (y * r.float().cuda()).sum().backward()
    errs = {"y": O.rel_l2(y.detach().cpu().double(), h.detach()), "gx": O.rel_l2(x.grad.cpu().double(), xr.grad)}
    for k, p in m.named_parameters():
        errs[k] = O.rel_l2(p.grad.cpu().double(), ps[k].grad)
    print(f"[split] {kind} {arg} T={T} slope {slope}: " + " ".join(f"{k.replace('conv_layers.', '')} {v:.1e}" for k, v in errs.items()))
    fwd_tol, g_tol = (5e-5, 1e-4) if slope == 1.0 else (1e-4, 2e-2)
    assert errs["y"] < fwd_tol, errs
    assert all(v < g_tol for k, v in errs.items() if k != "y"), {k: f"{v:.1e}" for k, v in errs.items()}


# ----------------------------------------------------------------------------------------------- the training shape
def test_split_equals_exact_at_training_shape(H):
    """Every sub-discriminator at the C3 discriminator-step shape (64 clips x 8192 samples): split against exact, both on the GPU,
    forward and every gradient.  This runs every tile variant the fp32 dispatcher picks at training sizes.  Forward measured
    2e-6 - 2.3e-5; the gradients (3-6e-3) carry the LeakyReLU kink flips of test_split_stack_vs_fp64 (exact and split disagree on the
    sign of a few pre-activations within ~1e-5 of zero), hence the 2e-2 bound."""
    torch.manual_seed(0)
    d = H.HiFiGANDiscriminators().cuda()
    torch.manual_seed(1)
    x = (torch.randn(64, 1, 8192) * 0.3).clamp(-1, 1).cuda()
    worst = {}
    for sub in list(d.mpd.discriminators) + list(d.msd.discriminators):
        res = {}
        for mode in ("exact", "split"):
            sub.set_fp32_operands(mode)
            sub.zero_grad(set_to_none=True)
            xi = x.clone().requires_grad_(True)
            y = sub(xi)
            torch.manual_seed(2)
            r = torch.randn(y.shape).cuda()
            (y * r).sum().backward()
            res[mode] = [y.detach()] + [xi.grad] + [p.grad.clone() for p in sub.parameters()]
        errs = [O.rel_l2(a.cpu().double(), b.cpu().double()) for a, b in zip(res["split"], res["exact"])]
        tag = f"p{sub.period}" if hasattr(sub, "period") else f"s{sub.scale}"
        worst[tag] = (errs[0], max(errs[1:]))
        sub.set_fp32_operands("exact")
    print("[split] vs exact at 64 x 8192, (forward, worst gradient): " + " ".join(f"{k} {a:.1e}/{b:.1e}" for k, (a, b) in worst.items()))
    assert all(a < 1e-4 and b < 2e-2 for a, b in worst.values()), worst


def test_exact_mode_is_the_generic_chain(H):
    """With no call to the switch an fp32 stack is bit for bit the generic Fn.conv2d / Fn.conv1d chain."""
    from hifigan_modified import functional as Fn
    torch.manual_seed(0)
    d = H.HiFiGANDiscriminators().cuda()
    assert d.fp32_operands == "exact" and all(s.fp32_operands == "exact" for s in d.modules() if hasattr(s, "conv_layers"))
    x = (torch.randn(2, 1, 1001) * 0.3).cuda()
    with torch.no_grad():
        for sub in d.mpd.discriminators:
            h = Fn._MpdFold.apply(x, sub.period)
            for li, c in enumerate(Fn._convs(sub.conv_layers)):
                h = Fn.conv2d(h, c.weight, c.bias, (1, 1), "lrelu" if li < 4 else None, 0.1)
            assert torch.equal(sub(x), h)
        for sub in d.msd.discriminators:
            h = Fn._AvgPool.apply(x, sub.scale) if sub.scale > 1 else x
            for li, c in enumerate(Fn._convs(sub.conv_layers)):
                h = Fn.conv1d(h, c.weight, c.bias, padding=7, act="lrelu" if li < 4 else None, slope=0.1)
            assert torch.equal(sub(x), h)


# ----------------------------------------------------------------------------------------------- training
def _trainer(H, use_graph, mode, dropout=0.0, seed=0, **kw):
    torch.manual_seed(seed)
    voc = H.ModifiedHiFiGANVocoder(dropout=dropout, **CFG)
    voc.discriminators.set_fp32_operands(mode)
    return H.VocoderTrainer(voc, device=torch.device("cuda"), use_graph=use_graph, **kw)


def _batch(i, B=2, T=64):
    g = torch.Generator().manual_seed(100 + i)
    return (torch.randn(B, 80, T, generator=g).cuda(), (torch.randn(B, 1, T * HOP, generator=g) * 0.5).clamp(-1, 1).cuda(),
            torch.randn(B, 192, generator=g).cuda(), torch.randn(B, 384, generator=g).cuda())


def _rel(a, b):
    return abs(a - b) / max(abs(a), 1e-12)


def test_split_training_tracks_exact(H):
    """12 steps of the small model from one seed and batches, split against exact discriminators (fp32 everywhere else)."""
    runs = {m: _trainer(H, True, m) for m in ("exact", "split")}
    hist = {m: [] for m in runs}
    for i in range(12):
        for m, t in runs.items():
            hist[m].append(t.train_step(*_batch(i % 5)))
    def worst(steps):
        return {k: max(_rel(hist["exact"][i][k], hist["split"][i][k]) for i in steps) for k in ("generator_loss", "discriminator_loss", "mel_loss")}
    w5, w12 = worst(range(5)), worst(range(12))
    print(f"[split] vs exact, worst relative loss difference over steps 0-4: {w5}; over steps 0-11: {w12}")
    assert all(v == v for o in hist["split"] for v in o.values())
    assert all(v < 1e-3 for v in w5.values()), w5


def _arenas(t):
    return [(o.flat_p, o.exp_avg, o.exp_avg_sq) for o in (t.generator_optimizer, t.discriminator_optimizer)]


def _sync_state(dst, src):
    """src's parameters and AdamW moments -> dst's arenas, in place (a captured graph keeps the arenas' addresses)."""
    from hifigan_modified import ops
    with torch.no_grad():
        for a, b in zip(_arenas(dst), _arenas(src)):
            for x, y in zip(a, b):
                x.copy_(y)
    ops.bump_param_epoch()


def _update_dist(t1, t2, before):
    """rel-L2 distance of two trainers' parameter arenas, relative to the update t1 made from `before`."""
    num = den = 0.0
    for a, b, p0 in zip(_arenas(t1), _arenas(t2), before):
        num += float((a[0].double() - b[0].double()).pow(2).sum())
        den += float((a[0].double() - p0.double()).pow(2).sum())
    return (num / den) ** 0.5


def test_captured_split_step_equals_eager(H):
    """Split mode, dropout 0.1, the counter RNG: the captured trainer against an eager one over six steps (two eager warm-up steps,
    the capture, three replays), a second eager trainer giving the noise floor.  The training kernels sum with fp32 atomics, so two
    runs differ by ~1e-7 from the first loss on, and over several steps AdamW's lr * sign(g) on near-zero gradients grows that into
    1e-5 - 1e-4 loss differences between ANY two trainers, two captured ones included; a six-step trajectory comparison is then a
    draw of that noise.  So every step starts all three trainers from the eager trainer's parameters and AdamW moments (copied into
    the arenas in place; step counts and the dropout counter advance on their own): each step's losses agree to one step's summation
    noise (measured <= 7e-7), and each step's parameter update to the eager-vs-eager spread of that update (measured: the first
    AdamW step, where near-zero gradients flip sign, 7e-4 against 8e-4 eager vs eager; later steps 1-2e-6)."""
    ta = _trainer(H, False, "split", dropout=0.1, dropout_rng="counter")
    tb = _trainer(H, True, "split", dropout=0.1, dropout_rng="counter")
    tc = _trainer(H, False, "split", dropout=0.1, dropout_rng="counter")
    for i in range(6):
        _sync_state(tb, ta)
        _sync_state(tc, ta)
        torch.cuda.synchronize()
        before = [o.flat_p.clone() for o in (ta.generator_optimizer, ta.discriminator_optimizer)]
        la, lb, lc = ta.train_step(*_batch(i)), tb.train_step(*_batch(i)), tc.train_step(*_batch(i))
        for k in la:
            assert _rel(la[k], lb[k]) < 2e-5 + 5 * _rel(la[k], lc[k]), (i, k, la, lb, lc)
        d_graph, d_eager = _update_dist(ta, tb, before), _update_dist(ta, tc, before)
        print(f"[split] step {i}: losses captured vs eager {max(_rel(la[k], lb[k]) for k in la):.1e}, eager vs eager "
              f"{max(_rel(la[k], lc[k]) for k in la):.1e}; update captured vs eager {d_graph:.1e}, eager vs eager {d_eager:.1e}")
        assert d_graph < 2e-3 + 3 * d_eager, (i, d_graph, d_eager)
    assert any(st["graph"] is not None for st in tb._graphs.values())
    for oa, ob in ((ta.generator_optimizer, tb.generator_optimizer), (ta.discriminator_optimizer, tb.discriminator_optimizer)):
        assert oa.steps == ob.steps and oa.step_count == ob.step_count == 6
    assert ta.dropout_rng.ctr_base == tb.dropout_rng.ctr_base > 0


def test_split_packs_follow_the_optimizer_step(H):
    """After an optimizer step the split stack must run on the UPDATED weights (its packed hi/lo images are refreshed)."""
    t = _trainer(H, False, "split")
    x = (torch.randn(2, 1, 64 * HOP) * 0.3).cuda()
    d = t.vocoder.discriminators
    with torch.no_grad():
        before = d.mpd.discriminators[0](x).clone()
    t.train_step(*_batch(0))
    with torch.no_grad():
        outs = {}
        for mode in ("split", "exact"):
            d.set_fp32_operands(mode)
            outs[mode] = [s(x) for s in list(d.mpd.discriminators) + list(d.msd.discriminators)]
    d.set_fp32_operands("split")
    assert not torch.equal(before, outs["split"][0])
    errs = [O.rel_l2(a.cpu().double(), b.cpu().double()) for a, b in zip(outs["split"], outs["exact"])]
    print(f"[split] after one step, split vs exact per sub-discriminator: {[f'{e:.1e}' for e in errs]}")
    assert max(errs) < 1e-4, errs


def test_opcheck_disc_conv_stack_fp32(H):
    from torch.library import opcheck
    ns = torch.ops.mi355x_vocoder
    g = lambda *s: (torch.randn(*s, device="cuda") * 0.2).requires_grad_(True)
    ch = (1, 32, 64, 128, 256, 1)
    for shp, k in (((2, 1, 3, 40), (3, 3)), ((2, 1, 50), (15,))):
        params = []
        for i in range(5):
            params += [g(ch[i + 1], ch[i], *k), g(ch[i + 1])]
        opcheck(ns.disc_conv_stack, (g(*shp), 0.1, *params), test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))
