"""The fused ODConv kernels of csrc/odconv_fused.hip, one dispatch arm at a time through the raw C ABI (mv_odconv_cl_pack,
mv_odconv_cl_fwd, _fwd_in16, _fwd_pair), against float64 torch on the CPU - bit for bit.  Inputs are small integers
(tests/odconv_cases.py), so every sum is exact in fp32 in any order and every result is representable in bf16, fp16 and fp32: one
wrong column, a dropped bias on one row block, a pooled_out slot written twice all change at least one element and fail
torch.equal.  The tables hold one base row per instantiation od_dispatch can select, with ragged companions and the generator's
routes to it; tests/test_host_odconv_cases.py proves on the host, against mv_odconv_cl_plan, that each row selects the arm it names.
The real-valued tests then bound every element by what the formats allow.

Worst observed error / bound of test_forward_real_values_elementwise on an MI355X, per arm (base row, LeakyReLU(0.1) and no
activation; the bound is derived in odconv_cases.real_bound, not fitted to these figures):
  bf16   kloop<2,3,1> 0.155, kloop<1,3,1> 0.057, cl<1,1,3,4> 0.362, cl<1,1,3,8> 0.238, cl<2,1,3,4> 0.645, cl<2,1,3,8> 0.661,
         sample<256,17> 0.181, mt<1,6,256> 0.215, cl<1,2,9,4> 0.101, cl<1,2,9,8> 0.116, mt<2,8,64> 0.179, mt<2,4,128> 0.143,
         cl<1,2,8,4> 0.449, cl<1,2,8,8> 0.446
  fp16   kloop<2,3,1> 0.124, kloop<1,3,1> 0.049, cl<1,1,3,4> 0.263, cl<1,1,3,8> 0.309, cl<2,1,3,4> 0.639, cl<2,1,3,8> 0.608,
         sample<256,17> 0.163, mt<1,6,256> 0.137, cl<1,2,9,4> 0.102, cl<1,2,9,8> 0.082, mt<2,8,64> 0.182, mt<2,4,128> 0.138,
         cl<1,2,8,4> 0.456, cl<1,2,8,8> 0.408
  fp32   kloop<2,3,2> 0.010, kloop<1,3,2> 0.003, cl<1,1,3,4> 0.162, cl<1,1,3,8> 0.056, cl<2,1,3,4> 0.232, cl<2,1,3,8> 0.250,
         cl<1,2,9,4> 0.025, cl<1,2,9,8> 0.016, stream<64,8,false> 0.008, stream<128,4,true> 0.003, mt<2,4,64> 0.024, mt<1,4,128> 0.016,
         mt<2,4,64,f16> 0.027, mt<1,4,128,f16> 0.011, cl<1,2,8,4> 0.178, cl<1,2,8,8> 0.122
The 16-bit figures are the one rounding of the stored output and of the mixed weight against a worst-case sum of magnitudes; the
largest belong to the 8-term base rows.  The fp32 figures are small where the sum is long (errors of random sign against a bound that
adds magnitudes).  The streaming arms are held to the constant of their own f16 hi + lo pieces (odconv_cases.C_STREAM, 3 * 2^-22
where the bf16 split has 3 * 2^-16); what is left of their bound is the worst-case fp32 summation term n 2^-24 A.
"""
import ctypes

import numpy as np
import pytest
import torch

import odconv_cases as C
from odconv_cases import ACT_LRELU, ACT_NONE, MV_BF16, MV_F16, MV_F32, TORCH_DT

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def L():
    from hifigan_modified import _native
    return _native.lib()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(t, dt):
    return t.to(TORCH_DT[dt] if isinstance(dt, int) else dt).cuda().contiguous()


def nans(shape, dtype):
    return torch.full(tuple(shape), float("nan"), dtype=TORCH_DT[dtype] if isinstance(dtype, int) else dtype, device="cuda")


def assert_same(got, want, what):
    """Bit equality of every element (as float64 on the CPU), with the first wrong elements named."""
    got = got.detach().double().cpu()
    want = want.double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if torch.equal(got, want):
        return
    bad = (got != want) | torch.isnan(got)
    idx = bad.nonzero()[:6].tolist()
    raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements differ; first (index, got, want): "
                         + "; ".join(f"{tuple(i)} {got[tuple(i)].item()} {want[tuple(i)].item()}" for i in idx))


def unpair(y):
    """Pair rows (f16 hi | f16 lo per 8-channel group, the byte size of the fp32 row) -> values, like _unpair of test_gpu_mrf_stream."""
    B, T, Cc = y.shape
    h = y.contiguous().view(torch.float16).view(B, T, Cc // 8, 2, 8).float()
    return (h[:, :, :, 0] + h[:, :, :, 1]).reshape(B, T, Cc)


def pack(L, w, c, param_dtype=torch.float32):
    """mv_odconv_cl_pack of the banks w [K, ...] held as `param_dtype` masters, into the storage type of the case."""
    n = L.mv_odconv_cl_packed_bytes(c.Cin, c.Cout, c.ks, c.stride, c.tr, c.K, c.dtype)
    assert n > 0
    buf = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    wd = w.to(param_dtype).cuda().contiguous()
    pdt = {torch.float32: MV_F32, torch.bfloat16: MV_BF16, torch.float16: MV_F16}[param_dtype]
    rc = L.mv_odconv_cl_pack(_p(wd), pdt, _p(buf), c.Cin, c.Cout, c.ks, c.stride, c.tr, c.K, c.dtype, _s())
    assert rc == 0, rc
    return buf


def x_dev(x, c):
    """The input in the type the entry point reads: the storage type, or fp16 for mv_odconv_cl_fwd_in16."""
    return dev(x, torch.float16 if c.in_f16 else c.dtype)


def launch(L, c, xd, pk, bias, alpha, y, pooled_out=None, act=ACT_NONE, slope=1.0, pooled_in=None, att_w=None, att_b=None, film=None,
           film_F=0, Tout=None, dtype=None):
    """The entry point of the case: mv_odconv_cl_fwd, or _fwd_in16 / _fwd_pair for the in_f16 / out_pair rows.  Returns the code."""
    g = C.geom_of(c)
    front = (_p(pk), _p(bias), _p(alpha), _p(pooled_in), 0 if pooled_in is None else pooled_in.shape[1], _p(att_w), _p(att_b))
    back = (_p(y), _p(pooled_out), c.B, c.Cin, c.Tin, c.Cout, g.Tout if Tout is None else Tout, c.ks, c.stride, c.pad, c.dil, c.tr, c.K, act,
            float(slope))
    if c.in_f16:
        return L.mv_odconv_cl_fwd_in16(_p(xd), *front, *back, _s())
    if c.out_pair:
        return L.mv_odconv_cl_fwd_pair(_p(xd), *front, *back, _s())
    return L.mv_odconv_cl_fwd(_p(xd), *front, _p(film), film_F, *back, c.dtype if dtype is None else dtype, _s())


def out_of(c, y):
    return unpair(y) if c.out_pair else y


def check_pooled(c, pooled, want_y, what):
    """pooled_out [B][slots][M]: every slot finite and written; summed over slots and stride phases it is the channel sum of y."""
    arm, g = C.arm_of(c), C.geom_of(c)
    p = pooled.double().cpu()
    assert bool(torch.isfinite(p).all()), f"{what}: {int((~torch.isfinite(p)).sum())} pooled_out elements not written"
    assert_same(p.view(c.B, arm.slots * (g.M // c.Cout), c.Cout).sum(1), C.pooled_ref(want_y), what + " pooled_out")


# =============================================================================================== forward, bit-exact
@pytest.mark.parametrize("c", C.CASES, ids=C.case_id)
def test_forward_exact(L, c):
    """y = act(conv(x; sum_k alpha_k W_k) + sum_k alpha_k bias_k) with and without bias, without activation and with LeakyReLU(0.5),
    behind an integer FiLM on the rows that carry one; pooled_out sums to the channel sums of y; fp32, bf16 and fp16 masters of the
    same integers pack to the same bytes."""
    shape, arm, g = C.shape_of(c), C.arm_of(c), C.geom_of(c)
    assert arm.name == c.arm
    x, w, b, alpha, ref = C.reference(shape)
    xd, bd, ad = x_dev(x, c), dev(b, c.dtype), dev(alpha, torch.float32)
    pk = pack(L, w, c)
    for pdt in (torch.bfloat16, torch.float16):
        assert torch.equal(pack(L, w, c, pdt), pk), f"{C.case_id(c)}: packed bytes from {pdt} masters differ"
    film_F = C.film_F_of(c.Cout) if c.film else 0
    film = C.film_inputs(c.B, c.Cout, film_F) if c.film else None
    fd = dev(film, c.dtype) if c.film else None
    for bias in (None, bd):
        want0 = ref if bias is None else ref + C.mixed_bias(alpha, b)
        if c.film:
            want0 = C.film_ref(want0, film, film_F)
        for act in (ACT_NONE, ACT_LRELU):
            want = want0 if act == ACT_NONE else C.lrelu(want0, C.SLOPE)
            y = nans((c.B, g.Tout, c.Cout), c.dtype)
            pooled = nans((c.B, arm.slots * g.M), torch.float32)
            what = f"{C.case_id(c)} bias={bias is not None} act={act}"
            assert launch(L, c, xd, pk, bias, ad, y, pooled, act, C.SLOPE, film=fd, film_F=film_F) == 0, what
            assert_same(out_of(c, y), want, what)
            check_pooled(c, pooled, want, what)
    if not c.film:                                           # without pooled_out: another epilogue instantiation of the cl kernels
        y = nans((c.B, g.Tout, c.Cout), c.dtype)
        assert launch(L, c, xd, pk, bd, ad, y, None, ACT_LRELU, C.SLOPE) == 0
        assert_same(out_of(c, y), C.lrelu(ref + C.mixed_bias(alpha, b), C.SLOPE), f"{C.case_id(c)} no pooled_out")


# =============================================================================================== impulses
@pytest.mark.parametrize("c", C.IMPULSE, ids=C.case_id)
def test_forward_impulses(L, c):
    """Per arm, on its row of odconv_cases.IMPULSE (several samples, row blocks and - where the arm can have them - column tiles):
    one non-zero input element at a time - the first and last column, both sides of the column-tile boundaries (of the 16-column
    blocks for the K-loop and sample-resident kernels, and of the spans a workgroup / a wave walks; on long walks the first, middle
    and last 16 positions), both sides of every 8-channel k-chunk boundary (every k-step and k-step block boundary is one), the last
    sample - must return the mixed kernel's taps around it and exact zeros elsewhere.  Then one non-zero bank weight at a time -
    the first and last GEMM row, both sides of every row-block boundary, every tap - must return alpha times the shifted input."""
    shape, arm, g = C.shape_of(c), C.arm_of(c), C.geom_of(c)
    _, w, _, alpha = C.inputs(shape)
    wb = torch.einsum("bk,k...->b...", alpha, w)
    pk, ad = pack(L, w, c), dev(alpha, torch.float32)
    xd = torch.zeros(c.B, c.Tin, c.Cin, dtype=torch.float16 if c.in_f16 else TORCH_DT[c.dtype], device="cuda")
    want = torch.zeros(c.B, g.Tout, c.Cout, dtype=torch.float32, device="cuda")
    for pt in C.x_impulses(c, arm, g):
        rows = C.x_impulse_rows(c, g, wb, pt)
        xd[pt] = 1.0
        for u, v in rows:
            want[pt[0], u] = v.float().cuda()
        y = nans((c.B, g.Tout, c.Cout), c.dtype)
        assert launch(L, c, xd, pk, None, ad, y) == 0
        if not torch.equal(out_of(c, y).float(), want):
            assert_same(out_of(c, y), want.cpu(), f"{C.case_id(c)} input impulse at {pt}")
        xd[pt] = 0.0
        for u, _ in rows:
            want[pt[0], u] = 0.0
    # weight impulses: a dense x in {-1, 0, 1}, all banks zero but one element of the bank the last sample weighs
    x = C.ints((c.B, c.Tin, c.Cin), -1, 1, 17)
    xd, xf = x_dev(x, c), x.float().cuda()
    kb = (c.B - 1) % c.K
    af = alpha.float().cuda()
    wz = torch.zeros(w.shape, dtype=torch.float32, device="cuda")
    n = L.mv_odconv_cl_packed_bytes(c.Cin, c.Cout, c.ks, c.stride, c.tr, c.K, c.dtype)
    pk = torch.empty(n, dtype=torch.uint8, device="cuda")
    for i, row in enumerate(C.row_edges(arm, g)):
        o, r = C.gemm_row_to_weight_index(c, row)
        for m in range(g.ntaps) if i < 4 else (i % g.ntaps,):      # every tap on the first rows, one tap (cycling) behind them
            j = r + m * c.stride if c.tr else m
            ch = (37 * row + 8 * m + 5) % c.Cin
            widx = (kb, ch, o, j) if c.tr else (kb, o, ch, j)
            wz[widx] = 1.0
            assert L.mv_odconv_cl_pack(_p(wz), MV_F32, _p(pk), c.Cin, c.Cout, c.ks, c.stride, c.tr, c.K, c.dtype, _s()) == 0
            u, t = C.w_impulse_steps(c, g, j)
            u, t = u.cuda(), t.cuda()
            want[:, u, o] = af[:, kb, None] * xf[:, t, ch]
            y = nans((c.B, g.Tout, c.Cout), c.dtype)
            assert launch(L, c, xd, pk, None, ad, y) == 0
            if not torch.equal(out_of(c, y).float(), want):
                assert_same(out_of(c, y), want.cpu(), f"{C.case_id(c)} weight impulse at GEMM row {row}, tap {m}, channel {ch}")
            wz[widx] = 0.0
            want[:, u, o] = 0.0


# =============================================================================================== the attention prologue, exact
def _first(pred):
    return next(c for c in C.CASES if pred(c))


ATT_CASES = [
    _first(lambda c: c.arm == "odconv_kloop_kernel<bf16,2,3,1>" and c.B % 2),                    # kloop, S = 2 with a missing sample
    _first(lambda c: c.arm == "odconv_kloop_kernel<float,1,3,2>"),
    _first(lambda c: c.arm == "odconv_cl_kernel<bf16,1,2,8,4>" and c.B > 1 and c.Cin == 64),     # cl, fast tail
    _first(lambda c: c.arm == "odconv_cl_kernel<f16,1,2,8,8>" and c.B > 1),                      # cl, general tail (K = 8)
    _first(lambda c: c.arm == "odconv_cl_kernel<float,2,1,3,8>" and c.B % 2),                    # cl, S = 2, K = 8
    _first(lambda c: c.arm == "odconv_cl_kernel<float,2,1,3,4>" and c.B % 2),                    # cl, S = 2, fast tail
    _first(lambda c: c.arm == "odconv_cl_kernel<bf16,1,1,3,8>" and c.Cin >= 512),                # cl, K = 8, wide input (Cin > 256)
    _first(lambda c: c.arm == "odconv_cl_kernel<f16,1,2,9,4>" and c.Cin == 512 and c.ks == 3),   # cl, fast tail, wide input
    _first(lambda c: c.arm == "odconv_cl_mt_kernel<f16,2,8,64>" and c.B > 1),
    _first(lambda c: c.arm == "odconv_cl_mt_kernel<bf16,1,6,256>" and c.B > 1),
    _first(lambda c: c.arm == "odconv_cl_mt_kernel<float,1,4,128>" and c.B > 1),
    _first(lambda c: c.arm == "odconv_cl_mt_kernel<float,2,4,64,f16>"),
    _first(lambda c: c.arm == "odconv_sample_kernel<bf16,256,17>"),
    _first(lambda c: c.arm == "odconv_stream_kernel<64,8,false>" and c.B > 1 and not c.out_pair),
    _first(lambda c: c.arm == "odconv_stream_kernel<64,8,false>" and c.out_pair),
    _first(lambda c: c.arm == "odconv_stream_kernel<128,4,true>" and c.B > 1),
]


@pytest.mark.parametrize("c", ATT_CASES, ids=C.case_id)
def test_attention_prologue_one_hot(L, c):
    """att_w = 0 and att_b = 0 on one bank, -1e4 on the others: the softmax is exactly one-hot (expf underflows to 0), so the output
    computed from pooled_in equals the explicit-alpha output bit for bit and the fp64 reference of that bank.  pooled_in carries
    three slots per channel of large values: read with a wrong stride or count they stay harmless only if multiplied by the zero
    weights, and anything non-finite would show."""
    shape, g = C.shape_of(c), C.geom_of(c)
    x, w, b, _, _ = C.reference(shape)
    xd, bd, pk = x_dev(x, c), dev(b, c.dtype), pack(L, w, c)
    pooled_in = (C.ints((c.B, 3 * c.Cin), -9, 9, 18) * 1e6).float().cuda()
    att_w = torch.zeros(c.K, c.Cin, dtype=TORCH_DT[c.dtype], device="cuda")
    for kb in sorted({0, c.K - 1, c.K // 2}):
        one_hot = torch.zeros(c.B, c.K, dtype=torch.float64)
        one_hot[:, kb] = 1.0
        att_b = torch.full((c.K,), -1e4, dtype=torch.float64)
        att_b[kb] = 0.0
        want = C.lrelu(C.odconv_ref(x, w, one_hot, shape, b), C.SLOPE)
        y1, y2 = nans((c.B, g.Tout, c.Cout), c.dtype), nans((c.B, g.Tout, c.Cout), c.dtype)
        assert launch(L, c, xd, pk, bd, dev(one_hot, torch.float32), y1, None, ACT_LRELU, C.SLOPE) == 0
        assert launch(L, c, xd, pk, bd, None, y2, None, ACT_LRELU, C.SLOPE, pooled_in=pooled_in, att_w=att_w, att_b=dev(att_b, c.dtype)) == 0
        assert_same(out_of(c, y1), want, f"{C.case_id(c)} explicit one-hot alpha, bank {kb}")
        assert torch.equal(y1.view(torch.uint8), y2.view(torch.uint8)), f"{C.case_id(c)}: pooled_in route differs, bank {kb}"


# =============================================================================================== real values, every element bounded
@pytest.mark.parametrize("c", C.BASE, ids=C.case_id)
def test_forward_real_values_elementwise(L, c):
    """x ~ N(0,1), banks and bank biases of a default-initialised ODConv module, softmax alpha, all rounded to the storage type
    (so the reference is computed in fp64 from exactly what the kernel is handed).  Every element:
        |y - act(ref)| <= c_T A + u_T |act(ref)| + n 2^-24 A,   A = sum_k |alpha_k| (sum |W_k| |x| + |bias_k|),
    u_T = 2^-8 (bf16), 2^-11 (fp16), 2^-24 (fp32): half an ulp of the stored significand; c_T = u_T for 16-bit storage (the one rounding of
    the mixed weight; the K-loop uses the stored banks as they are), 3 * 2^-16 + 2^-22 for fp32 (odconv_cases.C_OP: the two split
    representations and the dropped lo * lo product), for the streaming arms the same with f16 pieces (odconv_cases.C_STREAM); n = taps * Cin + 2 K + 2 fp32
    operations.  Derived, not measured."""
    g = C.geom_of(c)
    x, w, bias, alpha = C.real_inputs(c)
    ref, A, slack = C.real_bound(c, x, w, bias, alpha)
    xd, bd, ad, pk = x_dev(x, c), dev(bias, c.dtype), dev(alpha, torch.float32), pack(L, w, c)
    worst = 0.0
    for act, slope in ((ACT_LRELU, 0.1), (ACT_NONE, 1.0)):
        s32 = float(np.float32(slope))                      # the value the C ABI receives
        y = nans((c.B, g.Tout, c.Cout), c.dtype)
        assert launch(L, c, xd, pk, bd, ad, y, None, act, s32) == 0
        want = C.lrelu(ref, s32)
        err, bound = (out_of(c, y).double().cpu() - want).abs(), C.U[c.dtype] * want.abs() + slack
        if c.out_pair:
            bound = bound + 2.0 ** -22 * want.abs()         # the pair row keeps 22 bits of the fp32 value
        ratio = float((err / bound).max())
        worst = max(worst, ratio)
        assert bool((err <= bound).all()), (C.case_id(c), slope, ratio, int((err > bound).sum()))
    print(f"[odconv-real] {C.case_id(c)}: worst error / bound {worst:.3f}")


# =============================================================================================== refusals (nothing is launched)
def test_refusals_leave_the_outputs_alone(L):
    """Shapes the plan refuses return the same code from the launch entry points and write nothing: y and pooled_out keep their NaNs."""
    out = (ctypes.c_int * 14)()
    bad = [
        (C.Case("", 2, 64, 40, 64, 4, 2, 1, 1, 1, 4, 0, MV_F32, 1, 0, 0), "in_f16 with 3 column blocks"),
        (C.Case("", 2, 256, 100, 64, 4, 2, 1, 1, 1, 4, 0, MV_F32, 1, 0, 0), "in_f16 with 256 input channels"),
        (C.Case("", 2, 64, 100, 64, 3, 1, 1, 1, 0, 4, 0, MV_F32, 1, 0, 0), "in_f16 on a regular conv"),
        (C.Case("", 2, 64, 100, 32, 4, 2, 1, 1, 1, 4, 0, MV_F32, 0, 1, 0), "out_pair with Cout != 64"),
        (C.Case("", 2, 128, 100, 64, 4, 2, 1, 1, 1, 4, 0, MV_F32, 0, 1, 0), "out_pair with 128 input channels"),
        (C.Case("", 2, 64, 100, 64, 4, 2, 1, 1, 1, 8, 0, MV_F32, 0, 1, 0), "out_pair with 8 banks"),
        (C.Case("", 2, 64, 100, 8, 3, 1, 1, 1, 0, 4, 0, MV_BF16, 0, 0, 0), "M % 16 != 0"),
        (C.Case("", 2, 60, 100, 16, 3, 1, 1, 1, 0, 4, 0, MV_F16, 0, 0, 0), "Cin % 8 != 0"),
        (C.Case("", 2, 4096, 60, 16, 3, 1, 1, 1, 0, 1, 0, MV_F32, 0, 0, 0), "no tile of 4096 fp32 channels fits LDS"),
    ]
    for c, why in bad:
        with pytest.raises(C.Refused) as e:
            C.arm_of(c)
        try:
            Tout = C.geom_of(c).Tout
        except C.Refused:
            Tout = c.Tin * (c.stride if c.tr else 1)
        assert L.mv_odconv_cl_plan(c.B, c.Cin, c.Tin, c.Cout, Tout, c.ks, c.stride, c.pad, c.dil, c.tr, c.K, ACT_LRELU, 0, c.dtype,
                                   c.in_f16, c.out_pair, out) == e.value.code == C.MV_ERR_UNSUPPORTED, why
        xd = torch.ones(c.B, c.Tin, c.Cin, dtype=torch.float16 if c.in_f16 else TORCH_DT[c.dtype], device="cuda")
        pk = torch.zeros(1 << 22, dtype=torch.uint8, device="cuda")
        ad = torch.ones(c.B, c.K, device="cuda")
        y, pooled = nans((c.B, Tout, c.Cout), c.dtype), nans((c.B, 1 << 16), torch.float32)
        rc = _refused_launch(L, c, xd, pk, ad, y, pooled, Tout)
        assert rc == C.MV_ERR_UNSUPPORTED, (why, rc)
        torch.cuda.synchronize()
        assert bool(torch.isnan(y).all()) and bool(torch.isnan(pooled).all()), why
    # an unknown dtype on a valid shape
    c = C.Case("", 2, 64, 100, 64, 4, 2, 1, 1, 1, 4, 0, MV_F32, 0, 0, 0)
    xd, pk, ad = torch.ones(2, 100, 64, device="cuda"), torch.zeros(1 << 20, dtype=torch.uint8, device="cuda"), torch.ones(2, 4, device="cuda")
    y = nans((2, 200, 64), torch.float32)
    assert L.mv_odconv_cl_plan(2, 64, 100, 64, 200, 4, 2, 1, 1, 1, 4, ACT_LRELU, 0, 7, 0, 0, out) == C.MV_ERR_DTYPE
    assert launch(L, c, xd, pk, None, ad, y, dtype=7) == C.MV_ERR_DTYPE
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())


def _refused_launch(L, c, xd, pk, ad, y, pooled, Tout):
    """launch() for a shape whose geometry the restatement refuses to describe: Tout is passed as given."""
    front = (_p(pk), None, _p(ad), None, 0, None, None)
    back = (_p(y), _p(pooled), c.B, c.Cin, c.Tin, c.Cout, Tout, c.ks, c.stride, c.pad, c.dil, c.tr, c.K, ACT_LRELU, 0.5)
    if c.in_f16:
        return L.mv_odconv_cl_fwd_in16(_p(xd), *front, *back, _s())
    if c.out_pair:
        return L.mv_odconv_cl_fwd_pair(_p(xd), *front, *back, _s())
    return L.mv_odconv_cl_fwd(_p(xd), *front, None, 0, *back, c.dtype, _s())
