"""max_grad_norm clipping and the accumulating gather on FlatAdamW's gradient arena (optim.py; csrc/train.hip: mv_grad_norm,
mv_adamw_flat_clip, mv_multi_gather_acc, mv_zero_f32), at the optimizer level: hand-made fp32 parameters of 1, 7, 4099, 65537 and
3 x 5 x 7 elements - padding behind every parameter, a ragged last 16-byte group per parameter, more than one non-zero partial in the
norm - one of them without a gradient."""
import numpy as np
import pytest
import torch

from oracle import vocoder_oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [(1,), (7,), (4099,), (65537,), (3, 5, 7)]
NOGRAD = 1                      # the parameter that never receives a gradient
HP = dict(lr=1e-2, betas=(0.8, 0.99), weight_decay=1e-1)


@pytest.fixture(scope="module")
def H():
    import hifigan_modified as H
    from hifigan_modified import _native
    _native.lib()
    assert torch.cuda.is_available(), "GPU tests need cuda:0"
    return H


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=g).cuda()) for s in SHAPES]


def _grads(seed, scale=1.0):
    g = torch.Generator().manual_seed(1000 + seed)
    return [None if i == NOGRAD else torch.randn(*s, generator=g) * scale for i, s in enumerate(SHAPES)]


def _set(params, grads):
    for p, g in zip(params, grads):
        p.grad = None if g is None else g.to(p.device).clone()


def _norm64(grads):
    return float(torch.linalg.vector_norm(torch.cat([g.double().reshape(-1) for g in grads if g is not None])))


def _padding_mask(opt):
    pad = torch.ones(opt.numel, dtype=torch.bool)
    for p, o in zip(opt.params, opt.offsets):
        pad[o:o + p.numel()] = False
    return pad.cuda()


def test_grad_norm_matches_fp64_and_is_reproducible(H):
    """rel 1e-5: every term is non-negative, so the sum's relative error is at most (longest chain of dependent fp32 additions) x
    2^-24; the kernel states that chain as 34 (<= 300 gives 1.8e-5 on the sum, 0.9e-5 on its root)."""
    from hifigan_modified.optim import FlatAdamW
    ps = _params()
    opt = FlatAdamW(ps, **HP)
    grads = _grads(0)
    _set(ps, grads)
    opt.gather_grads()
    ns = torch.ops.mi355x_vocoder
    ref = _norm64(grads)
    buf = opt._clip_slots()
    bits = []
    for max_norm, pre in ((0.5 * ref, 1.0), (0.5 * ref, 1.0), (1e9, 1.0), (1.0, 0.25)):
        ns.grad_norm(opt.flat_g, buf, None, max_norm, pre)
        norm, coef = (float(v) for v in buf[:2].cpu())
        bits.append(buf[:2].cpu().view(torch.int32).tolist())
        print(f"[grad_norm] max_norm {max_norm:.4g} pre_scale {pre}: norm {norm!r} (fp64 {pre * ref!r}, rel {abs(norm - pre * ref) / (pre * ref):.2e}) coef {coef!r}")
        assert abs(norm - pre * ref) <= 1e-5 * pre * ref
        want = min(1.0, max_norm / (pre * ref + 1e-6))
        assert abs(coef - want) <= 2e-5 * want
        if max_norm == 1e9:
            assert coef == 1.0
    assert bits[0] == bits[1]                                   # the same input, the same bits
    # max_norm from device memory (what a captured step reads) gives the bits of the by-value form
    mx = torch.tensor([0.5 * ref], dtype=torch.float32, device="cuda")
    ns.grad_norm(opt.flat_g, buf, mx, 0.0, 1.0)
    assert buf[:2].cpu().view(torch.int32).tolist() == bits[0]
    # a slice whose length is no multiple of 4 (the tail path), at a 16-byte aligned start
    sl = opt.flat_g[16:16 + 4099]
    ns.grad_norm(sl, buf, None, 1.0, 1.0)
    r = float(torch.linalg.vector_norm(sl.double()))
    assert abs(float(buf[0]) - r) <= 1e-5 * r
    # non-finite gradients: torch's coefficients (error_if_nonfinite=False)
    g2 = opt.flat_g.clone()
    g2[5] = float("inf")
    ns.grad_norm(g2, buf, None, 1.0, 1.0)
    assert float(buf[0]) == float("inf") and float(buf[1]) == 0.0
    g2[5] = float("nan")
    ns.grad_norm(g2, buf, None, 1.0, 1.0)
    assert torch.isnan(buf[:2]).all()


@pytest.mark.parametrize("factor", [0.5, 2.0, None])
def test_clipped_step_matches_torch_clip_grad_norm(H, factor):
    """Three steps against torch.optim.AdamW + clip_grad_norm_ on fp32 CPU clones (tolerance of the unclipped parity test,
    test_gpu_train_parity.py: rel-L2 1e-6 per parameter); where the coefficient is 1 the arena is bit-equal to step() without
    max_grad_norm from the same state."""
    from hifigan_modified.optim import FlatAdamW
    ps, ps_plain = _params(), _params()
    ref = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps]
    opt, opt_plain = FlatAdamW(ps, **HP), FlatAdamW(ps_plain, **HP)
    topt = torch.optim.AdamW(ref, **HP)
    max_norm = 1e9 if factor is None else factor * _norm64(_grads(0))
    for it in range(3):
        grads = _grads(it)
        _set(ps, grads)
        _set(ps_plain, grads)
        _set(ref, grads)
        opt.step(max_grad_norm=max_norm)
        opt_plain.step()
        tn = torch.nn.utils.clip_grad_norm_(ref, max_norm)
        topt.step()
        assert abs(float(opt.grad_norm) - float(tn)) <= 1e-5 * float(tn)
        coef = float(opt._clip_buf[1])
        assert (coef == 1.0) == (factor != 0.5), (factor, coef)
    for i, (p, q) in enumerate(zip(ps, ref)):
        if i == NOGRAD:
            assert torch.equal(p.detach().cpu(), q.detach())          # untouched, bit for bit
        else:
            assert O.rel_l2(p.detach().cpu(), q.detach()) < 1e-6, i
    assert opt.steps == [0 if i == NOGRAD else 3 for i in range(len(SHAPES))] and opt.step_count == 3
    same = all(torch.equal(a, b) for a, b in ((opt.flat_p, opt_plain.flat_p), (opt.exp_avg, opt_plain.exp_avg),
                                              (opt.exp_avg_sq, opt_plain.exp_avg_sq)))
    if factor == 0.5:
        assert not same                                               # the clip really changed the update
    else:
        assert same
    assert opt_plain.grad_norm is None and opt_plain._clip_buf is None    # max_grad_norm=None: no norm, no buffer


def test_device_hyperparameter_form_of_the_clipped_update(H):
    """The captured step's form (hyper-parameters and step count from device memory): coefficient 1 gives the bits of
    fused_adamw_hp_, coefficient c the bits of fused_adamw_hp_ on a gradient scale of grad_scale * c."""
    ns = torch.ops.mi355x_vocoder
    n = 4099
    g = torch.Generator().manual_seed(5)
    mk = lambda: [torch.randn(n, generator=g).cuda() for _ in range(2)] + [torch.rand(n, generator=g).cuda() * 0.1 for _ in range(2)]
    base = mk()
    hp = torch.tensor([1e-2, 0.8, 0.99, 1e-8, 1e-1], device="cuda")
    step = torch.tensor([3], dtype=torch.int32, device="cuda")
    for c, gs in ((1.0, 0.5), (0.37, 0.5)):
        a, b = [t.clone() for t in base], [t.clone() for t in base]
        coef = torch.tensor([c], dtype=torch.float32, device="cuda")
        ns.fused_adamw_clip_(a[0], a[1], a[2], a[3], hp, step, 0.0, 0.0, 0.0, 0.0, 0.0, 0, gs, coef)
        ns.fused_adamw_hp_(b[0], b[1], b[2], b[3], hp, step, float(np.float32(gs) * np.float32(c)))
        assert all(torch.equal(x, y) for x, y in zip(a, b)), c


def test_accumulating_gather(H):
    """Gather A, then accumulate B: A + B exactly (one fp32 add per element), nothing added for a missing gradient, padding words
    stay zero; zero_arena() starts a window from zero."""
    from hifigan_modified.optim import FlatAdamW
    ps = _params()
    opt = FlatAdamW(ps, **HP)
    pad = _padding_mask(opt)
    A, B = _grads(1), _grads(2)
    B[3] = None                                  # the 65537-element parameter has no gradient in the second gather
    _set(ps, A)
    opt.gather_grads()
    assert opt._has_grad == [i != NOGRAD for i in range(len(SHAPES))]
    _set(ps, B)
    flat = opt.gather_grads(accumulate=True).clone()
    assert opt._has_grad == [i != NOGRAD for i in range(len(SHAPES))]           # the OR over the window
    for i, (p, o) in enumerate(zip(opt.params, opt.offsets)):
        got = flat[o:o + p.numel()].cpu()
        want = torch.zeros(p.numel()) if A[i] is None else A[i].reshape(-1).clone()
        if B[i] is not None:
            want = want + B[i].reshape(-1)
        assert torch.equal(got, want), i
    assert float(flat[pad].abs().max()) == 0.0
    # a window from zero: zero_arena, then two accumulating gathers (parameter NOGRAD still never has one)
    opt.zero_arena()
    assert float(opt.flat_g.abs().max()) == 0.0 and opt._has_grad == [False] * len(SHAPES)
    _set(ps, A)
    opt.gather_grads(accumulate=True)
    _set(ps, B)
    opt.gather_range(0, 3, accumulate=True)
    opt.gather_range(3, 5, accumulate=True)
    assert torch.equal(opt.flat_g, flat)
    assert opt._has_grad == [i != NOGRAD for i in range(len(SHAPES))]
    opt.step(grad_scale=0.5, gathered=True, max_grad_norm=1.0)     # a gradient in ANY gather of the window counts
    assert opt.steps == [0 if i == NOGRAD else 1 for i in range(len(SHAPES))]


def _table(srcs, offsets):
    from hifigan_modified import ops
    from hifigan_modified.optim import _DESC
    d = np.zeros(len(srcs), dtype=_DESC)
    for i, (s, o) in enumerate(zip(srcs, offsets)):
        d["dst_off"][i] = o
        d["n"][i] = 7 if s is None else s.numel()
        if s is not None:
            d["src"][i], d["dtype"][i] = s.data_ptr(), ops._DT[s.dtype]
    return torch.from_numpy(d.view(np.uint8).reshape(-1).copy()).cuda(), int(d["n"].max())


def test_accumulating_gather_widens_16bit_sources_exactly(H):
    ns = torch.ops.mi355x_vocoder
    g = torch.Generator().manual_seed(7)
    srcs = [torch.randn(4099, generator=g).cuda().bfloat16(), None, torch.randn(65537, generator=g).cuda().half(),
            torch.randn(33, generator=g).cuda()]
    offsets = [0, 4104, 4112, 4112 + 65544]
    flat = torch.randn(offsets[-1] + 40, generator=g).cuda()
    before = flat.clone()
    table, max_len = _table(srcs, offsets)
    ns.multi_gather_acc_(table, len(srcs), max_len, flat)
    want = before.clone()
    for s, o in zip(srcs, offsets):
        if s is not None:
            want[o:o + s.numel()] += s.float()
    assert torch.equal(flat, want)               # 16-bit -> fp32 is exact, then one fp32 add; everything else untouched


def test_opcheck_new_operators(H):
    from torch.library import opcheck
    from hifigan_modified.torch_ops import GRAD_NORM_WS_WORDS
    ns = torch.ops.mi355x_vocoder
    tests = ("test_schema", "test_faketensor")
    c = lambda *s: torch.randn(*s, device="cuda")
    srcs = [c(40), c(9).bfloat16()]
    table, max_len = _table(srcs, [0, 40])
    opcheck(ns.multi_gather_acc_, (table, 2, max_len, c(56)), test_utils=tests)
    opcheck(ns.zero_, (c(56),), test_utils=tests)
    buf = torch.zeros(2 + GRAD_NORM_WS_WORDS, device="cuda")
    opcheck(ns.grad_norm, (c(4099), buf, None, 1.0, 1.0), test_utils=tests)
    opcheck(ns.grad_norm, (c(64), buf, torch.ones(1, device="cuda"), 0.0, 0.5), test_utils=tests)
    p_, g_, m_, v_ = c(64), c(64), torch.zeros(64, device="cuda"), torch.zeros(64, device="cuda")
    coef = torch.full((1,), 0.5, device="cuda")
    opcheck(ns.fused_adamw_clip_, (p_, g_, m_, v_, None, None, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, 1.0, coef), test_utils=tests)
    hp = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 0.01], device="cuda")
    opcheck(ns.fused_adamw_clip_, (p_, g_, m_, v_, hp, torch.ones(1, dtype=torch.int32, device="cuda"), 0.0, 0.0, 0.0, 0.0, 0.0, 0, 1.0, coef),
            test_utils=tests)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ns.zero_(torch.zeros(8))
