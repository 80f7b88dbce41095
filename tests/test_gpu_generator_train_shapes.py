"""Generator backward at the shapes the trainer runs (B = 32 clips x 32 mel frames, hidden 512, upsample factors [8, 8, 2, 2], MRF at
64 channels over 8192 samples), against fp64 autograd of the oracle (oracle/vocoder_oracle.py) on the same rounded operands.

The kernels pick their work split from B, T and the channel counts, so the small shapes of test_gpu_grads.py take other branches.
The branches pinned here, each named at the test that reaches it:
  1. mv_conv1d_wgrad per-sample direct store (tsplit == 1, no zero fill) next to the zero-then-atomicAdd path;
  2. the MFMA ODConvTranspose bank gradient with several 128-position chunks per sample (halo into the next chunk and into the
     padded row Tin), the adjoint data gradient over long rows, and output_padding = 1;
  3. the MFMA 1-row weight gradient with several chunks per workgroup (the MRF merged k11 conv and 1x1 fusion conv at T = 8192,
     the MSD k15 layers in test_gpu_train_fullsize.py);
  4. GroupNorm backward over 8192-step rows, vector and scalar (T % 8 != 0) paths;
  5. the per-sample attention chain (galpha, the pooling term 1/T Wa^T gz) at B = 32;
  6. the fp32-storage generic kernels at full channel counts.

Every comparison is of gradients (not optimizer updates).  Parameters are kept in fp32 (as the trainer keeps them) but rounded to the
storage type in place, so the kernels and the reference read identical values; the input and the cotangent r are rounded the same way.
The fp64 references run on the GPU (torch's native fp64 convolutions, not this package's kernels): on the CPU the B = 32 upsampler
references alone take minutes.  Bounds: fp32 storage 2e-4 per tensor (1e-3 for one-element tensors), the convention of
test_gpu_grads.py; 16-bit bounds are 2-3x the error measured on the MI355X (both numbers at each table)."""
import pytest
import torch

from backward_cases import wgrad_tsplit as _wgrad_tsplit     # host rule of mv_conv1d_wgrad: time chunks per (sample, tile); 1 = direct store
from oracle import vocoder_oracle as O

pytestmark = pytest.mark.gpu
REF = "cuda"          # fp64 reference device
F32_TOL, F32_TOL_SCALAR = 2e-4, 1e-3


@pytest.fixture(scope="module")
def H():
    import hifigan_modified as H
    from hifigan_modified import _native
    _native.lib()
    return H


def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _round_params_(mod, dtype):
    """fp32 parameters rounded in place to `dtype` values: the kernels' cast and the reference then see the same numbers."""
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(p.to(dtype).float())
    return mod


def _ref_params(mod, names):
    return {k: p.detach().to(REF, torch.float64).requires_grad_(True) for k, p in mod.named_parameters() if k in names}


def _check(errs, tols, tag):
    print(f"[gen-train] {tag}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    bad = {k: f"{v:.2e} > {tols[k]:.0e}" for k, v in errs.items() if not v < tols[k]}
    assert not bad, (tag, bad)


def _cotangent(shape, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(shape, device="cuda", generator=g).to(dtype)


def odconv_transpose_fp64(m, x, r, stride, padding, output_padding=0):
    """fp64 reference of ODConvTranspose1d (odconv.py:172-205): alpha = softmax(Wa mean_t x + ba), y = sum_k alpha_k (convT(x, W_k) +
    b_k), and the gradients of sum(y * r).  Returns (y, x.grad, {parameter name: grad}) in fp64 on x's device."""
    names = ("kernels", "bias", "kernel_attention.1.weight", "kernel_attention.1.bias")
    sd = {k: p.detach().to(x.device, torch.float64).requires_grad_(True) for k, p in m.named_parameters() if k in names}
    xr = x.detach().double().requires_grad_(True)
    yr = O.odconv_transpose1d(xr, sd, "", stride=stride, padding=padding, output_padding=output_padding)
    (yr * r.double()).sum().backward()
    return yr.detach(), xr.grad, {k: v.grad for k, v in sd.items()}


def _run_odconv_transpose(H, dtype, cin, cout, ks, stride, pad, opad, Tin, B, seed=0):
    """GPU forward/backward of one ODConvTranspose1d and its fp64 reference: (errors, spy record of the fused launches)."""
    torch.manual_seed(seed)
    m = H.ODConvTranspose1d(cin, cout, ks, stride=stride, padding=pad, output_padding=opad)
    with torch.no_grad():
        m.bias.normal_(0, 0.1)
    md = _round_params_(m.cuda(), dtype).train(False)
    gen = torch.Generator(device="cuda").manual_seed(seed + 1)
    x = torch.randn(B, cin, Tin, device="cuda", generator=gen).to(dtype)
    fz, seen = md._fused(), {}
    if dtype != torch.float32:        # record what the fused MFMA launchers returned (None = fell back to the generic kernels)
        for name in ("dgrad", "wgrad"):
            orig = getattr(fz, name)
            setattr(fz, name, lambda *a, _o=orig, _n=name: seen.setdefault(_n, []).append(_o(*a)) or seen[_n][-1])
    xd = x.clone().requires_grad_(True)
    y = md(xd)
    r = _cotangent(y.shape, dtype, seed + 2)
    (y.float() * r.float()).sum().backward()
    yr, gxr, gp = odconv_transpose_fp64(md, x.to(REF), r.to(REF), stride, pad, opad)
    assert y.shape == yr.shape
    errs = {"y": O.rel_l2(y, yr), "y[0]": O.rel_l2(y[0], yr[0]), f"y[{B - 1}]": O.rel_l2(y[-1], yr[-1]),
            "gx": O.rel_l2(xd.grad, gxr), "gx[0]": O.rel_l2(xd.grad[0], gxr[0]), f"gx[{B - 1}]": O.rel_l2(xd.grad[-1], gxr[-1])}
    for k, p in md.named_parameters():
        if k in gp:
            errs[k] = O.rel_l2(p.grad, gp[k])
        else:
            assert p.grad is None, k          # the constructed-but-unused attention heads
    del m, md, x, xd, y, r, yr, gxr, gp
    for name in list(seen):
        delattr(fz, name)
    _free()
    return errs, {k: [v is not None for v in vs] for k, vs in seen.items()}


# ---------------------------------------------------------------------------------------------------------------- A
# (cin, cout, ks, stride, pad, output_padding, Tin, B); ids name the generator layer whose geometry it is
_UPS = [
    pytest.param(512, 256, 16, 8, 4, 0, 32, 32, id="ups0"),
    pytest.param(256, 128, 16, 8, 4, 0, 256, 32, id="ups1"),
    pytest.param(128, 64, 4, 2, 1, 0, 2048, 8, id="ups2-B8"),
    pytest.param(128, 64, 4, 2, 1, 0, 2048, 32, id="ups2-B32"),
    pytest.param(64, 64, 4, 2, 1, 0, 4096, 8, id="ups3"),
    pytest.param(128, 64, 8, 4, 2, 0, 2048, 8, id="ups2-48k"),
    pytest.param(128, 64, 4, 2, 1, 0, 129, 8, id="ragged129"),
    pytest.param(256, 128, 16, 8, 4, 0, 1000, 4, id="ragged1000"),
    pytest.param(128, 64, 6, 3, 1, 1, 300, 8, id="odd-op1"),
]
# rel-L2 bounds; measured on MI355X, max over the shapes above (whole tensor and per sample alike):
#   output / x.grad: one rounding of the 16-bit result - bf16 2.4e-3 / 2.9e-3, fp16 2.9e-4 / 3.7e-4
#   bank, bias and attention-head gradients: fp32 sums of exactly representable products - <= 1.0e-6 in both types
_UPS_TOL = {torch.bfloat16: dict(y=6e-3, gx=6e-3, w=3e-6), torch.float16: dict(y=8e-4, gx=8e-4, w=3e-6)}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("cin,cout,ks,stride,pad,opad,Tin,B", _UPS)
def test_odconv_transpose_mfma_training_shapes(H, dtype, cin, cout, ks, stride, pad, opad, Tin, B):
    """Items 2 and 5: the 16-bit upsampler backward on the MFMA route - data gradient as the adjoint two-tap ODConv over rows of
    `stride` steps (mv_odconv_cl_fwd), bank gradients as per-sample two-tap weight-gradient GEMMs (dwgrad_launch<T,2>, chunk WT = 128,
    xW = Tin + 1: Tin >= 129 puts two or more chunks in every sample and the halo across each chunk edge), then the alpha chain.
    Output and x.grad per sample (first and last: the per-sample attention and pooling term) and whole; the bank, bias and
    attention-head gradients sum over the batch and are compared whole."""
    from hifigan_modified.fused import OdconvFused
    torch.manual_seed(0)
    assert OdconvFused(H.ODConvTranspose1d(cin, cout, ks, stride=stride, padding=pad, output_padding=opad)).dgrad_supported()
    errs, seen = _run_odconv_transpose(H, dtype, cin, cout, ks, stride, pad, opad, Tin, B)
    assert seen == {"dgrad": [True], "wgrad": [True]}, seen       # both adjoint ops ran on the MFMA kernels
    t = _UPS_TOL[dtype]
    tols = {k: t["y"] if k.startswith("y") else t["gx"] if k.startswith("gx") else t["w"] for k in errs}
    _check(errs, tols, f"odconvT {dtype} {cin}->{cout} k{ks} s{stride} Tin{Tin} B{B}")


# ---------------------------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("cin,cout,ks,stride,pad,Tin,B,direct", [
    pytest.param(512, 256, 16, 8, 4, 32, 4, True, id="ups0-B4"),
    pytest.param(256, 128, 16, 8, 4, 256, 16, True, id="ups1-B16"),
    pytest.param(256, 128, 16, 8, 4, 256, 4, False, id="ups1-B4"),
])
def test_odconv_transpose_fp32_storage_full_channels(H, cin, cout, ks, stride, pad, Tin, B, direct):
    """Items 1 and 6: fp32-storage upsamplers at ups0 / ups1 channel counts on the generic kernels - the data gradient as conv1d with
    alpha, the bank gradients from mv_conv1d_wgrad with the roles of input and gradient swapped (tiles = (cout/16) x (cin/16) over Tin
    positions), on both of its store paths: tiles * B >= 2048 (or Tin <= 64) is the per-sample direct store, fewer tiles the
    zero-then-atomicAdd split.  Measured <= 1.6e-6 on every tensor (bound 2e-4)."""
    assert (_wgrad_tsplit(B, cout, cin, Tin) == 1) == direct
    errs, seen = _run_odconv_transpose(H, torch.float32, cin, cout, ks, stride, pad, 0, Tin, B)
    _check(errs, {k: F32_TOL for k in errs}, f"odconvT fp32 {cin}->{cout} Tin{Tin} B{B} {'direct' if direct else 'atomics'}")


# ---------------------------------------------------------------------------------------------------------------- B
# (output and x.grad, parameter gradients); measured: bf16 2.4e-3 / 9e-7, fp16 3.0e-4 / 9e-7, fp32 1.1e-6 / 5e-7
_INP_TOL = {torch.bfloat16: (6e-3, 3e-6), torch.float16: (8e-4, 3e-6), torch.float32: (F32_TOL, F32_TOL)}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_input_projection_odconv1d_both_wgrad_stores(H, dtype):
    """Items 1, 5 and 6: the input projection ODConv1d(80 -> 512, k7, K = 4).  Its bank gradient runs on mv_conv1d_wgrad in every
    storage type (160 tiles of 16 x 16): at B = 32, Tm = 32 the per-sample direct store (5120 tile-samples, no zero fill of the
    workspace), at B = 2, Tm = 256 the time split with fp32 atomics - both against the same fp64 reference.  The input requires a
    gradient here (in the generator it is the leaf mel batch), so the data gradient and the pooling term run too."""
    names = ("kernels", "bias", "kernel_attention.1.weight", "kernel_attention.1.bias")
    for B, Tm, direct in ((32, 32, True), (2, 256, False)):
        assert (_wgrad_tsplit(B, 80, 512, Tm) == 1) == direct
        torch.manual_seed(0)
        m = H.ODConv1d(80, 512, 7, padding=3, K=4, reduction_factor=4)
        with torch.no_grad():
            m.bias.normal_(0, 0.1)
        md = _round_params_(m.cuda(), dtype).train(False)
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn(B, 80, Tm, device="cuda", generator=g).to(dtype)
        xd = x.clone().requires_grad_(True)
        y = md(xd)
        r = _cotangent(y.shape, dtype, 2)
        (y.float() * r.float()).sum().backward()
        sd = _ref_params(md, names)
        xr = x.to(REF, torch.float64).requires_grad_(True)
        yr = O.odconv1d(xr, sd, "", padding=3)
        (yr * r.to(REF).double()).sum().backward()
        errs = {"y": O.rel_l2(y, yr), "y[0]": O.rel_l2(y[0], yr[0]), f"y[{B - 1}]": O.rel_l2(y[-1], yr[-1]),
                "gx": O.rel_l2(xd.grad, xr.grad), "gx[0]": O.rel_l2(xd.grad[0], xr.grad[0]),
                f"gx[{B - 1}]": O.rel_l2(xd.grad[-1], xr.grad[-1])}
        for k, p in md.named_parameters():
            if k in sd:
                errs[k] = O.rel_l2(p.grad, sd[k].grad)
            else:
                assert p.grad is None, k
        tols = {k: _INP_TOL[dtype][0 if k.startswith(("y", "gx")) else 1] for k in errs}
        _check(errs, tols, f"input_proj {dtype} B{B} Tm{Tm} {'direct' if direct else 'atomics'}")
        del m, md, x, xd, y, r, sd, xr, yr
        _free()


# ---------------------------------------------------------------------------------------------------------------- D
# measured (max over both shapes): output / x.grad bf16 2.8e-3 / 3.1e-3, fp16 3.5e-4 / 3.9e-4, fp32 2.0e-7 / 1.8e-7; other tensor
# gradients bf16 1.1e-2, fp16 6.8e-4, fp32 1.3e-6; the scalar lora_scaling gradients bf16 1.53, fp16 0.23, fp32 4.4e-4
_MRF_TOL = {torch.bfloat16: dict(y=8e-3, gx=8e-3, p=2.5e-2, scalar=3.0),
            torch.float16: dict(y=1e-3, gx=1e-3, p=1.5e-3, scalar=0.5),
            torch.float32: dict(y=F32_TOL, gx=F32_TOL, p=F32_TOL, scalar=F32_TOL_SCALAR)}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("T,B", [(8192, 8), (8191, 2)])
def test_mrf_block_generator_geometry(H, dtype, T, B):
    """Items 3, 4 and 6: MultiReceptiveFieldBlock(64, 64) as the generator builds it, training path, dropout off.  16-bit: the merged
    branch conv (64 -> 120, k11) and the 1x1 fusion conv (60 -> 64) take their weight gradients from the MFMA 1-row kernel; at
    T = 8192 a sample is 64 chunks of 128 positions, B = 8 gives 512 chunks over 2 x 64 tile groups (4 chunks per workgroup, across
    sample boundaries).  GroupNorm backward reduces 8 or 5 channels x 8192 steps per (sample, group); T = 8191 takes the scalar
    path and a ragged last chunk.  fp32 runs the generic kernels.  Output, x.grad and every parameter gradient."""
    from hifigan_modified import functional as Fn
    torch.manual_seed(0)
    m = H.MultiReceptiveFieldBlock(64, 64).train(False)
    md = _round_params_(m.cuda(), dtype)
    sd = {k: v.detach().to(REF, torch.float64).requires_grad_(True) for k, v in md.state_dict().items()}
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(B, 64, T, device="cuda", generator=g).to(dtype)
    xd = x.clone().requires_grad_(True)
    assert Fn._mrf_merged_ok(xd, md) == (dtype != torch.float32)
    y = md(xd)
    r = _cotangent(y.shape, dtype, 2)
    (y.float() * r.float()).sum().backward()
    xr = x.to(REF, torch.float64).requires_grad_(True)
    yr = O.mrf_block(xr, sd, "", (1, 3, 5))
    (yr * r.to(REF).double()).sum().backward()
    t = _MRF_TOL[dtype]
    errs = {"y": O.rel_l2(y, yr), "gx": O.rel_l2(xd.grad, xr.grad)}
    tols = {"y": t["y"], "gx": t["gx"]}
    for k, p in md.named_parameters():
        ref = sd[k].grad
        assert p.grad is not None and ref is not None, k
        errs[k] = O.rel_l2(p.grad, ref)
        # lora_scaling is ONE scalar: a cancelling sum over B x T x 20 x 64 products of the 16-bit branch gradient, whose
        # rounding noise grows with B x T while the sum does not (fp16 / bf16 errors scale with the rounding unit, 0.23 / 1.53;
        # test_gpu_grads.py measures 10 % / 24 % at T = 700) - rounding, not a kernel defect.  In bf16 the bound carries no
        # information; the fp32 and fp16 runs of this test pin the scalar.
        tols[k] = t["scalar"] if ref.numel() == 1 else t["p"]
    _check(errs, tols, f"mrf {dtype} T{T} B{B}")
    del m, md, sd, x, xd, y, r, xr, yr
    _free()


# ---------------------------------------------------------------------------------------------------------------- E
# Two tiers in 16-bit storage.  Gradients that pass the LeakyReLU of an upsampler ("kink": the stages input_proj .. up2 and the
# parameters of input_proj, FiLM and the upsamplers) carry kink-flip noise: a pre-activation within 16-bit rounding of 0 takes the
# other slope, and the flipped fraction costs ~sqrt(fraction) in rel-L2 (it jumps from up3 to up2 and scales with the square root
# of the rounding unit: bf16 / fp16 = 2.9x).  Everything behind the last LeakyReLU (up3, the MRF blocks, the output conv) is smooth.
# Measured (max over the tier): kink bf16 9.5e-2, fp16 3.5e-2; smooth bf16 1.6e-2, fp16 1.8e-3; the scalar lora_scaling gradients
# (cancelling sums, see test_mrf_block_generator_geometry) bf16 0.58, fp16 4.7e-2; fp32 2.2e-6 (scalars 1.2e-4).
_GEN_TOL = {torch.bfloat16: dict(kink=0.2, smooth=4e-2, scalar=1.5), torch.float16: dict(kink=8e-2, smooth=4e-3, scalar=0.12),
            torch.float32: dict(kink=F32_TOL, smooth=F32_TOL, scalar=F32_TOL_SCALAR)}
_KINK = ("input_proj", "film", "final_film.", "up0", "up1", "up2", "upsample_layers.")


def _gen_tier(name):
    return "kink" if any(name == "grad." + s or name.startswith(s) for s in _KINK) else "smooth"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_default_generator_stage_and_parameter_gradients(H, dtype):
    """The whole default generator (hidden 512, [8, 8, 2, 2], speaker + emotion conditioning, dropout 0) at B = 2, Tm = 32 -> 8192
    samples: the gradient reaching every stage output (input_proj, film, up0..up3, mrf0..mrf2, wave) and every parameter gradient
    against fp64 autograd of oracle.generator_forward; the unused attention heads stay grad-less.  output_proj.weight is scaled by
    0.05 on both sides: at random init tanh saturates ~97 % of the samples and would zero most of the upstream gradient."""
    torch.manual_seed(0)
    gen = H.ModifiedHiFiGANGenerator(dropout=0.0)
    with torch.no_grad():
        gen.output_proj.weight.mul_(0.05)
    gd = _round_params_(gen.cuda(), dtype).train(False)
    sd = {k: v.detach().to(REF, torch.float64).requires_grad_(True) for k, v in gd.state_dict().items()}
    g = torch.Generator(device="cuda").manual_seed(1)
    mel = torch.randn(2, 80, 32, device="cuda", generator=g).to(dtype)
    spk = torch.randn(2, 192, device="cuda", generator=g).to(dtype)
    emo = torch.randn(2, 256, device="cuda", generator=g).to(dtype)
    st = gd(mel, spk, emo, return_stages=True)
    for v in st.values():
        v.retain_grad()
    wave = st["wave"]
    assert wave.shape == (2, 1, 8192)
    sat = float((wave.detach().float().abs() > 0.95).float().mean())
    assert sat < 0.05, sat
    r = _cotangent(wave.shape, dtype, 2)
    (wave.float() * r.float()).sum().backward()
    ref = O.generator_forward(mel.to(REF).double(), sd, "", spk.to(REF).double(), emo.to(REF).double(), return_stages=True)
    for v in ref.values():
        v.retain_grad()
    (ref["wave"] * r.to(REF).double()).sum().backward()
    t = _GEN_TOL[dtype]
    errs, tols = {}, {}
    for k, v in st.items():
        errs["grad." + k] = O.rel_l2(v.grad, ref[k].grad)
        tols["grad." + k] = t[_gen_tier("grad." + k)]
    errs["wave"], tols["wave"] = O.rel_l2(wave, ref["wave"]), t["smooth"]
    n = 0
    for k, p in gd.named_parameters():
        rg = sd[k].grad
        if rg is None:
            assert p.grad is None, f"{k} must stay grad-less (unused in the reference)"
            continue
        assert p.grad is not None, k
        errs[k] = O.rel_l2(p.grad, rg)
        tols[k] = t["scalar"] if rg.numel() == 1 else t[_gen_tier(k)]
        n += 1
    assert n > 100
    print(f"[gen-train] generator {dtype}: saturated {sat:.3f}")
    _check(errs, tols, f"generator {dtype}")
    del gen, gd, sd, st, wave, ref
    _free()
