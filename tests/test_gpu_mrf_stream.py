"""MRF chain in the two-product operand mode (MV_F32_W16) and its streaming form (csrc/mrf_stream.hip).

Reference arithmetic: hifigan_modified/grc_lora.py:32-68 (GRC_LoRA_Block), :157-163 (MultiReceptiveFieldBlock.forward), checked
through the oracle (oracle/vocoder_oracle.py, pinned to the reference's goldens).  Tolerances: the mode rounds the folded MRF
weights to f16 once (2^-12 relative): ~1.5e-4 rel-L2 per block on random inputs, +1.1e-4 in quadrature on the C2 waveform
(tools/error_budget.py); north_star's bound on the waveform is 1e-3 and is asserted at the full C2 size below."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import vocoder_oracle as O  # noqa: E402
from numerics_sim import mrf_blocks  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    import hifigan_modified as H
    return H


def _blocks(H, seed=0):
    blks, sds = mrf_blocks(seed)                              # shared with tests/test_gpu_inference_off_unit_scale.py
    return [bk.cuda().train(False) for bk in blks], sds


@pytest.mark.parametrize("B,T", [(2, 48), (3, 700), (1, 16), (1, 17), (5, 1000), (2, 4100), (2, 8192)])
def test_stream_chain_vs_oracle_ragged(H, B, T):
    """1, 2 and 3 chained blocks on ragged shapes: against the oracle's blocks, bit-reproducible, and close to the three-product tile
    form of the same chain.  What these shapes reach (mv_mrf_plan, tests/test_host_mrf_plan.py): a partial last column tile, waves
    without work, several workgroups per sample - and ONE-tile spans only: every shape plans tpw = 1, L = 16 in the streaming form
    and nit = 1 in the tile form, so the ring of three slots never wraps and no workgroup walks a second tile here.  Multi-tile
    spans, spans that end inside a column tile and workgroups with idle iterations are in tests/test_gpu_mrf_arms.py."""
    from hifigan_modified.fused import MrfChain, mrf_fused_for
    blks, sds = _blocks(H)
    chain = MrfChain([mrf_fused_for(bk) for bk in blks])
    torch.manual_seed(T)
    x = torch.randn(B, 64, T)
    xc = x.cuda().transpose(1, 2).contiguous()
    with torch.no_grad():
        ref, refs = x[:2], []
        for sd in sds:
            ref = O.mrf_block(ref, sd, "")
            refs.append(ref)
        for n in (1, 2, 3):
            y = chain.forward_cl(xc, n, w16=True)
            y2 = chain.forward_cl(xc, n, w16=True)
            assert torch.equal(y, y2)
            e = O.rel_l2(y.transpose(1, 2)[:2].cpu(), refs[n - 1])
            assert e < 4e-4, (n, e)                       # measured 1.5e-4 / 2.1e-4 / 2.4e-4
            full = chain.forward_cl(xc, n)                # three-product mode (bf16 x 3): the parity-grade chain
            assert O.rel_l2(y.cpu(), full.cpu()) < 4e-4


@pytest.mark.parametrize("arm", ["tile_form", "ks17"])
def test_w16_chain_arms_beside_the_streaming_form(H, arm):
    """The two arms of the chain's dispatcher (csrc/mrf_fused.hip, mrf_chain_run) that no other test reaches in the two-product mode,
    at B = 2, T = 200 (ragged against every tile width), two blocks, against the fp64 oracle:
      tile_form  dilations (1, 2, 4): not the streaming form's (1, 3, 5), so mv_mrf_chain_fwd_cl runs mrf_kernel<f32w16> and its pass F;
      ks17       mv_mrf_chain_out_fwd_cl with a 17-tap output conv: beyond the 16 MFMA rows of the form that takes the last block's
                 partial sums, so the chain runs in its tile form, mrf_affine_kernel writes the deferred affine and the fp32 VALU
                 output conv applies it.  The head is linear here (ACT_NONE): what is compared is the chain's output seen through an
                 fp32 conv (its own rounding: 2^-24 per term), not a saturated tanh.
    Bound: the 4e-4 of test_stream_chain_vs_oracle_ragged, the existing test of this storage mode (single-f16 weights: ~1.5e-4 per
    block); the tile form keeps fp32 rows between the blocks, so it has no rounding the streaming form lacks."""
    import ctypes
    import torch.nn.functional as F
    from hifigan_modified import _native as N, ops
    from hifigan_modified.fused import MrfChain, mrf_fused_for
    dil = (1, 2, 4) if arm == "tile_form" else (1, 3, 5)
    blks, sds = mrf_blocks(0, dilations=dil)
    chain = MrfChain([mrf_fused_for(bk.cuda().train(False)) for bk in blks[:2]])
    torch.manual_seed(200)
    x = torch.randn(2, 64, 200)
    xc = x.cuda().transpose(1, 2).contiguous()
    with torch.no_grad():
        ref = x.double()
        for sd in sds[:2]:
            ref = O.mrf_block(ref, {k: v.double() for k, v in sd.items()}, "", dilations=dil)
        if arm == "tile_form":
            y = chain.forward_cl(xc, 2, w16=True)
            assert torch.equal(y, chain.forward_cl(xc, 2, w16=True))
            got = y.transpose(1, 2).cpu()
        else:
            torch.manual_seed(3)
            w = (torch.randn(1, 64, 17) * (2.0 / 17) ** 0.5).cuda()
            wt = torch.empty(N.lib().mv_conv_out_packed_bytes(64, 17), device="cuda", dtype=torch.uint8)
            N.call("mv_conv_out_pack_all", ctypes.c_void_p(w.data_ptr()), ops._DT[w.dtype], ctypes.c_void_p(wt.data_ptr()), 64, 17, ops._stream())
            got = chain.forward_out_cl(xc, wt, 0.25, 17, N.ACT_NONE, w16=True).cpu()
            assert got.shape == (2, 1, 200)
            ref = F.conv1d(ref, w.cpu().double(), torch.tensor([0.25], dtype=torch.float64), padding=8)
    e = O.rel_l2(got, ref)
    print(f"[w16-arms] {arm}: rel-L2 vs fp64 oracle {e:.3e}")
    assert e < 4e-4, (arm, e)


def test_full_c2_batch_mixed_w16_meets_north_star(H):
    """bench.py's headline mode at BASELINE configs[1]'s full size: fp16 storage through up1, fp32 storage behind it, the three MRF
    blocks with two-product operands (streaming chain + fused output conv).  Four of the 32 clips against the oracle within
    north_star's 1e-3 waveform rel-L2 (measured 6.3e-4 over the full batch, per-clip maximum 7.7e-4), fp32 output, two runs agree
    bit for bit; the 48 kHz geometry refuses the mode's claim (tools/error_budget.py: 1.5e-3 there) by staying opt-in."""
    torch.manual_seed(0)
    gen = H.ModifiedHiFiGANGenerator()
    sd = {k: v.detach().clone() for k, v in gen.state_dict().items()}
    gen = gen.cuda().train(False).set_mixed_precision("up1", mrf_weights="fp16")
    torch.manual_seed(1)
    mel, spk, emo = torch.randn(32, 80, 32), torch.randn(32, 192), torch.randn(32, 384)
    with torch.no_grad():
        wave = gen(mel.cuda(), spk.cuda(), emo.cuda())
        again = gen(mel.cuda(), spk.cuda(), emo.cuda())
        assert wave.shape == (32, 1, 8192) and wave.dtype == torch.float32 and torch.equal(wave, again)
        errs = []
        for i in (0, 7, 13, 31):
            ref = O.generator_forward(mel[i:i + 1], sd, "", spk[i:i + 1], emo[i:i + 1])
            errs.append(O.rel_l2(wave[i:i + 1].cpu(), ref))
        print(f"[parity] mixed through up1 + MRF two-product operands: waveform rel-L2 vs oracle {[f'{e:.2e}' for e in errs]}")
        assert max(errs) < 1e-3, errs
        # stage outputs of the same mode go through the materialising chain entry (mv_mrf_chain_fwd_cl)
        # (a batch of 2 sums its GroupNorm partials in another grouping than the batch of 32: 1e-7 differences, which the 15-bit rows
        #  between the blocks turn into an occasional flipped last bit - the two runs agree to the rows' rounding level, not to fp32's)
        st = gen(mel[:2].cuda(), spk[:2].cuda(), emo[:2].cuda(), return_stages=True)
        e2 = O.rel_l2(st["wave"].cpu(), wave[:2].cpu())
        print(f"[parity] stage-wise entry, batch of 2, vs the fused batch of 32: {e2:.2e}")
        assert e2 < 1e-4
    with pytest.raises(ValueError):
        gen.set_mixed_precision("up1", mrf_weights="bf16")


def test_graph_replay_survives_eager_call_at_another_shape(H):
    """A captured forward bakes the chain's workspace pointer into the HIP graph; an eager call at another shape in between must not
    free that workspace (round-2 advisor finding: the cache used to keep one workspace and replace it)."""
    from hifigan_modified.graphs import GraphedVocoder
    torch.manual_seed(0)
    gen = H.ModifiedHiFiGANGenerator().cuda().train(False).set_mixed_precision("up1", mrf_weights="fp16")
    torch.manual_seed(1)
    mel, spk, emo = torch.randn(4, 80, 32).cuda(), torch.randn(4, 192).cuda(), torch.randn(4, 384).cuda()
    with torch.no_grad():
        want = gen(mel, spk, emo).clone()
        gv = GraphedVocoder(gen, mel, spk, emo)
        assert torch.equal(gv.replay(), want)
        for tm in (8, 16, 5):                               # other (B, T): new workspaces, new intermediate tensors
            gen(torch.randn(1, 80, tm).cuda(), spk[:1], emo[:1])
        junk = [torch.randn(1 << 22, device="cuda") for _ in range(8)]     # recycle whatever the allocator may have freed
        del junk
        torch.cuda.synchronize()
        assert torch.equal(gv.replay(), want)


def _pair_rows(x_cl):
    """fp32 [B, T, 64] -> the chain's pair rows (per 8-channel group: 8 f16 hi, 8 f16 lo), as an fp32-typed tensor of the same shape."""
    B, T, C = x_cl.shape
    g = x_cl.view(B, T, C // 8, 8)
    hi = g.to(torch.float16)
    lo = (g - hi.float()).to(torch.float16)
    return torch.stack([hi, lo], dim=3).contiguous().view(torch.float32).view(B, T, C)


def _unpair(y):
    B, T, C = y.shape
    h = y.contiguous().view(torch.float16).view(B, T, C // 8, 2, 8).float()
    return (h[:, :, :, 0] + h[:, :, :, 1]).reshape(B, T, C)


@pytest.mark.parametrize("B,T", [(2, 48), (3, 700), (1, 17), (2, 4100)])
def test_stream_chain_takes_pair_rows(H, B, T):
    """MV_F32_W16P: the chain fed with its own row format (what the last upsampler's streaming kernel writes) - the first pass reads it
    by LDS-DMA - equals the chain fed with fp32 rows up to the representation of the rows (one block: the 22-bit input, 2^-22
    relative - plus f as a 15-bit hl8 row on the fp32-row side; more blocks: both of that side's streams are hl8 rows, 2^-15)."""
    from hifigan_modified.fused import MrfChain, mrf_fused_for
    blks, _ = _blocks(H)
    chain = MrfChain([mrf_fused_for(bk) for bk in blks])
    torch.manual_seed(T + 1)
    xc = torch.randn(B, T, 64, device="cuda")
    with torch.no_grad():
        for n in (1, 3):
            a = chain.forward_cl(xc, n, w16=True)
            b = chain.forward_cl(_pair_rows(xc), n, w16=True, x_pair=True)
            b2 = chain.forward_cl(_pair_rows(xc), n, w16=True, x_pair=True)
            assert torch.equal(b, b2)
            # (the fp32-row entry keeps its streams between the blocks as 15-bit hl8 rows, the pair-row entry as 22-bit pair rows)
            assert O.rel_l2(b.cpu(), a.cpu()) < (1e-5 if n == 1 else 1e-4), (n, O.rel_l2(b.cpu(), a.cpu()))


@pytest.mark.parametrize("B,T", [(2, 64), (3, 1000), (32, 4096)])
def test_last_upsampler_writes_pair_rows(H, B, T):
    """mv_odconv_cl_fwd_pair: the 64 -> 64 channel ODConvTranspose1d (x2) of the generator writes the chain's pair rows; decoded
    (hi + lo) they are the fp32 output of the same kernel to 2^-22, and the channel sums handed on are the same numbers."""
    from hifigan_modified import functional as Fn, ops
    from hifigan_modified import _native as N
    from hifigan_modified.fused import OdconvFused
    torch.manual_seed(5)
    m = H.ODConvTranspose1d(64, 64, 4, stride=2, padding=1).cuda()
    with torch.no_grad():
        m.bias.copy_(torch.randn_like(m.bias) * 0.5)
    fz = OdconvFused(m)
    x = torch.randn(B, T, 64, device="cuda")
    pooled = x.sum(dim=1).contiguous()
    n = fz.pool_floats(B, T, torch.float32, N.ACT_LRELU)
    with torch.no_grad():
        p1 = torch.full((B, n), float("nan"), device="cuda")
        p2 = torch.full((B, n), float("nan"), device="cuda")
        y = fz.forward_cl(x, Fn._cache, pooled_in=pooled, pooled_out=p1, act=N.ACT_LRELU)
        yp, is_pair = fz.forward_cl(x, Fn._cache, pooled_in=pooled, pooled_out=p2, act=N.ACT_LRELU, out_pair=True)
    assert is_pair and yp.shape == y.shape
    assert float((_unpair(yp) - y).abs().max()) <= 2.0 ** -21 * float(y.abs().max())
    assert torch.equal(p1, p2)
