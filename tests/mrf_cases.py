"""Case tables and host-side restatement for the fused MultiReceptiveFieldBlock kernels (csrc/mrf_fused.hip: tile form,
csrc/mrf_stream.hip: streaming form, csrc/conv_out.hip: the chain's fused ending) - a plain module, imported like
tests/disc_cases.py and tests/odconv_cases.py by tests/test_host_mrf_plan.py (no GPU) and tests/test_gpu_mrf_arms.py.

It restates, in Python, what the host code decides from (entry, B, T, dilations, dtype): the tap table of a dilation set
(mrf_make_meta), the work split of the tile form (mrf_geometry: nit tiles per workgroup) and of the streaming form (sr_geometry: tpw
column tiles per wave), the fp32 chain's wide first pass, the dynamic LDS of every pass, the way a chain ends and what the output conv
reads.  The library answers the same question through mv_mrf_plan (the dry run of its launchers); the host test holds the two against
each other.  It also holds the per-column error the GPU test bounds and the batch builder of its inputs."""
import torch

MV_OK, MV_ERR_ARG, MV_ERR_DTYPE, MV_ERR_UNSUPPORTED = 0, -1, -2, -3
MV_F32, MV_BF16, MV_F16, MV_F32_W16, MV_F32_W16P = 0, 1, 2, 3, 4
DT_NAME = {MV_F32: "fp32", MV_BF16: "bf16", MV_F16: "fp16", MV_F32_W16: "w16", MV_F32_W16P: "w16_pair"}

ENTRY_BLOCK, ENTRY_CHAIN, ENTRY_CHAIN_PASSES, ENTRY_CHAIN_OUT = 0, 1, 2, 3
MATERIALIZE, PASSES_ONLY, TAIL_WITH_AB, TAIL_WITH_PARTIALS = 0, 1, 2, 3
ROWS_NONE, ROWS_FP32, ROWS_PAIR, ROWS_HL8 = -1, 0, 1, 4
OUT_NONE, OUT_AFFINE, OUT_AFFINE_MFMA = -1, 0, 1

PLAN_FIELDS = ("form", "nwaves", "ntw", "std_mask", "nwg", "nit", "wide", "tpw", "L", "lds", "lds_wide", "lds_stat", "gx", "gy", "kind",
               "out_family", "row_form", "launches", "hmax", "out_lds")

MRF_HMAX = 8
LDS_MAX = 160 * 1024
FRAG_BYTES = 1024
CONV_FRAGS, RES_FRAGS, FUS_FRAGS = 32, 8, 8
TAB_BYTES = 7 * 64 * 4
STD = (1, 3, 5)

# operand type of the tile form -> (weight images per fragment, storage element size): Mma<T>::NSETS, ::ES (csrc/mfma.h)
_MMA = {"float": (2, 4), "f32w16": (1, 4), "bf16": (1, 2), "f16": (1, 2)}
# storage dtype -> the instantiations <T, NWAVES, NTW> its dispatcher tries, in order (mv_mrf_block_fwd_cl, mrf_chain_run)
TILE_ARMS = {MV_F32: (("float", 8, 1), ("float", 4, 2)), MV_F32_W16: (("f32w16", 8, 2),), MV_BF16: (("bf16", 8, 4),),
             MV_F16: (("f16", 8, 4),)}
# time steps of the workgroup tile, NWAVES x NTW x 16: what the issue's table calls the 128-, 512- and 256-step tile
TILE_T = {MV_F32: 128, MV_BF16: 512, MV_F16: 512, MV_F32_W16: 256}

SR_NW, SR_RING, SR_H = 8, 3 * 16 * 272, 5


class Refused(Exception):
    def __init__(self, code):
        super().__init__(code)
        self.code = code


def cdiv(a, b):
    return -(-a // b)


def make_meta(dil):
    """mrf_make_meta: (ntaps, halo, is_std) of a dilation set, or None where the fused kernels do not take it."""
    offs = {0}
    for d in dil:
        if not 1 <= d <= 8:
            return None
        offs |= {d, -d}
    if len(offs) > 7:
        return None
    offs = sorted(offs)
    pairs = 0                                      # fragment pairs: per 16-row M-tile, the taps its branches use
    for mt in range(4):
        used = set()
        for row in range(16 * mt, min(16 * mt + 16, 60)):
            d = dil[row // 20]
            used |= {0, d, -d}
        pairs += len(used)
    if 2 * pairs > CONV_FRAGS:
        return None
    return len(offs), max(dil), tuple(dil) == STD


def mrf_geometry(B, T, tile_t):
    """mrf_geometry: (nwg, nit) - up to 8 tiles per workgroup while the grid stays above 256 workgroups."""
    ntiles = cdiv(T, tile_t)
    it = 1
    while it < 8 and B * cdiv(ntiles, it) > 256 and cdiv(ntiles, it * 2) >= 1 and ntiles >= it * 2:
        it *= 2
    return cdiv(ntiles, it), it


def sr_geometry(B, T):
    """sr_geometry: (tpw, L, nwg) - column tiles and time steps of a wave's span, workgroups per sample."""
    tiles = cdiv(T, 16)
    wgs = max(256 // B, 1)
    tpw = max(cdiv(tiles, wgs * SR_NW), 1)
    return tpw, tpw * 16, cdiv(tiles, tpw * SR_NW)


def sr_lds(full):
    return (48 if full else 32) * FRAG_BYTES + TAB_BYTES + (32 + 16 + SR_NW * 32) * 4 + 512 * 8 + SR_NW * SR_RING


def tile_plan(arm, metas, chain, B, T):
    """mrf_tile_plan for one instantiation: dict of the tile-form fields, or Refused(MV_ERR_UNSUPPORTED)."""
    Tn, nwaves, ntw = arm
    nsets, es = _MMA[Tn]
    fs = nsets * FRAG_BYTES
    rs = (2 * 64 * 2 if es == 4 else 64 * es) + 32
    nwg, nit = mrf_geometry(B, T, nwaves * ntw * 16)
    hmax = max(m[1] for m in metas)
    rows = nwaves * ntw * 16 + 2 * hmax if es == 4 else nwaves * (ntw * 16 + 2 * hmax)
    fixed = TAB_BYTES + (32 + 16) * 4 + nwaves * 32 * 4
    lds = (CONV_FRAGS + RES_FRAGS + FUS_FRAGS) * fs + fixed + rows * rs
    if lds > LDS_MAX or hmax > MRF_HMAX:
        raise Refused(MV_ERR_UNSUPPORTED)
    lds_wide = CONV_FRAGS * fs + fixed + (nwaves * 2 * 16 + 2 * hmax) * rs
    wide = bool(chain and es == 4 and ntw == 1 and nit >= 2 and nit % 2 == 0 and lds_wide <= LDS_MAX and T % (nwaves * 32) == 0)
    return dict(form=0, nwaves=nwaves, ntw=ntw, std_mask=sum(1 << i for i, m in enumerate(metas) if m[2]), nwg=nwg, nit=nit, wide=int(wide),
                tpw=0, L=0, lds=lds, lds_wide=lds_wide if wide else 0, lds_stat=0, gx=nwg, gy=B, kind=-1, out_family=OUT_NONE,
                row_form=ROWS_NONE, launches=0, hmax=hmax, out_lds=0)


def _first_arm(dtype, metas, chain, B, T):
    err = None
    for arm in TILE_ARMS[dtype]:
        try:
            return tile_plan(arm, metas, chain, B, T)
        except Refused as e:
            err = e
    raise err


def plan(entry, B, T, dils, dtype, ks=7):
    """What mv_mrf_plan must answer for valid pointers: the plan as a dict of PLAN_FIELDS, or Refused(code).  dils: one dilation set
    per block."""
    n = len(dils)
    if not (B > 0 and B <= 65535 and T > 0 and 1 <= n <= 8) or (entry == ENTRY_BLOCK and n != 1):
        raise Refused(MV_ERR_ARG)
    if entry == ENTRY_CHAIN_OUT and not (ks > 0 and ks & 1):
        raise Refused(MV_ERR_ARG)
    metas = [make_meta(d) for d in dils]
    if any(m is None for m in metas):
        raise Refused(MV_ERR_UNSUPPORTED)
    if entry == ENTRY_BLOCK:
        if dtype not in (MV_F32, MV_BF16, MV_F16):
            raise Refused(MV_ERR_DTYPE)
        p = _first_arm(dtype, metas, False, B, T)
        p["launches"] = 3
        return p
    pair_in = dtype == MV_F32_W16P
    sdt = MV_F32_W16 if pair_in else dtype
    if sdt not in TILE_ARMS:
        raise Refused(MV_ERR_DTYPE)
    cdt = MV_F32 if sdt == MV_F32_W16 else sdt                      # the output conv sees fp32 storage either way
    partials = cdt == MV_F32 and ks <= 16
    kind = {ENTRY_CHAIN: MATERIALIZE, ENTRY_CHAIN_PASSES: PASSES_ONLY}.get(entry, TAIL_WITH_PARTIALS if partials else TAIL_WITH_AB)
    p = None
    if sdt == MV_F32_W16:
        if all(m[2] for m in metas) and kind != TAIL_WITH_AB and T * 256 < 2 ** 31:
            tpw, L, nwg = sr_geometry(B, T)
            p = dict(form=1, nwaves=SR_NW, ntw=1, std_mask=(1 << n) - 1, nwg=nwg, nit=0, wide=0, tpw=tpw, L=L, lds=sr_lds(True), lds_wide=0,
                     lds_stat=sr_lds(False), gx=nwg, gy=B, kind=kind, out_family=OUT_NONE, row_form=ROWS_NONE,
                     launches=2 * n + (kind == MATERIALIZE), hmax=SR_H, out_lds=0)
            rows = ROWS_PAIR if pair_in else ROWS_HL8 if n > 1 else ROWS_FP32
        elif pair_in:
            raise Refused(MV_ERR_UNSUPPORTED)                      # only the streaming form reads pair rows
    if p is None:
        p = _first_arm(sdt, metas, True, B, T)
        p["kind"] = kind
        p["launches"] = 2 * n + (kind in (MATERIALIZE, TAIL_WITH_AB))
        rows = ROWS_FP32
    if entry == ENTRY_CHAIN_OUT:
        if partials:
            p.update(out_family=OUT_AFFINE_MFMA, out_lds=cdiv(256 + ks - 1, 16) * 16 * (2 * 64 * 2 + 16))
        else:
            out_lds = (256 + ks - 1) * (64 * (4 if cdt == MV_F32 else 2) + 16)
            if out_lds > LDS_MAX:
                raise Refused(MV_ERR_UNSUPPORTED)
            p.update(out_family=OUT_AFFINE, out_lds=out_lds)
        p["row_form"] = rows
        p["launches"] += 1
    return p


# ------------------------------------------------------------------------------------------------ shapes and arms
# The ragged shapes of the MRF tests that existed before these tables: every one takes the one-tile-per-worker split in every form.
OLD_RAGGED = ((2, 48), (3, 700), (1, 16), (1, 17), (5, 1000), (2, 4100), (2, 8192), (4, 8192))

# Split shapes: the smallest found that reach each loop.  Per form (fp32 tile 128 steps, 16-bit tile 512, w16 tile 256, streaming):
# the fields the plan must show, and in words what the shape reaches inside the kernel.
SPLIT_SHAPES = ((40, 3684), (40, 3584), (130, 600))
SPLIT_ARMS = {
    # 29 fp32 tiles: 4 workgroups x 8, the last with 5 (three empty iterations), last tile 100 steps; 8 16-bit tiles: 4 x 2;
    # 15 w16 tiles: 4 x 4, one idle iteration; streaming: 231 column tiles, spans of 5 (ring of 3 slots wraps), one span of 4 steps
    # (ends inside a column tile), one idle wave in the last of 6 workgroups
    (40, 3684): {"fp32": dict(nit=8, nwg=4, wide=0), "16bit": dict(nit=2, nwg=4), "w16_tile": dict(nit=4, nwg=4),
                 "stream": dict(tpw=5, L=80, nwg=6)},
    # 28 fp32 tiles, T % 256 == 0: the chain's first pass is wide over nit / 2 = 4 iterations, and the last workgroup (4 tiles) runs 2
    (40, 3584): {"fp32": dict(nit=8, nwg=4, wide=1), "16bit": dict(nit=2, nwg=4), "w16_tile": dict(nit=4, nwg=4),
                 "stream": dict(tpw=5, L=80, nwg=6)},
    # 5 fp32 tiles: 2 workgroups x 4, the last with one tile and three idle iterations; 2 16-bit tiles in one workgroup; streaming:
    # one workgroup per sample, 38 column tiles in spans of 5: the last wave has 3
    (130, 600): {"fp32": dict(nit=4, nwg=2, wide=0), "16bit": dict(nit=2, nwg=1), "w16_tile": dict(nit=2, nwg=2),
                 "stream": dict(tpw=5, L=80, nwg=1)},
}

DIL_SHAPES = ((2, 200), (3, 700))
DIL_SETS = ((1, 2, 4), (1, 1, 2), (1, 3, 7), (2, 4, 8))          # (1, 1, 2): the fewest taps; (1, 3, 7): halo 7; (2, 4, 8): halo MRF_HMAX


def seam_distance(t, plan_fields, T):
    """Distance of column t to the nearest boundary between two workers' spans (a wave's span in the streaming form, a wave's
    NTW x 16-step tile in the tile form), in time steps; the ends of the sample count as boundaries too."""
    step = plan_fields["L"] if plan_fields["form"] == 1 else plan_fields["ntw"] * 16
    return min(min(t % step, step - 1 - t % step), T - 1 - t)


# ------------------------------------------------------------------------------------------------ inputs and the metric
def base_clips(T, seed=None):
    """Three seeded clips [3, 64, T] fp32."""
    g = torch.Generator().manual_seed(1000 + T if seed is None else seed)
    return torch.randn(3, 64, T, generator=g)


def tile_batch(base, B):
    """x[i] = base[i % 3]: a batch of B built from three distinct clips."""
    return base[torch.arange(B) % base.shape[0]].contiguous()


def column_error(y, ref):
    """e[b, t] = ||y[b, :, t] - ref[b, :, t]||_2 / sqrt(mean_t ||ref[b, :, t]||_2^2), in fp64; y, ref [B, C, T]."""
    y, ref = y.double(), ref.double()
    rms = ref.pow(2).sum(1).mean(1).sqrt()
    return (y - ref).pow(2).sum(1).sqrt() / rms[:, None]


def rel_l2(y, ref):
    y, ref = y.double(), ref.double()
    return float((y - ref).norm() / ref.norm())


MARGIN = 1.5                    # GPU per-column maximum <= MARGIN x the simulation's (tests/test_gpu_inference_off_unit_scale.py)
THREE_COL, THREE_GLOBAL = 5e-5, 2e-5      # three-product fp32: 2e-5 (test_mrf_fused_vs_generic_and_golden) x 2.5, maximum over rms of noise
GLOBAL_BOUND = {"w16": 4e-4, "w16_pair": 4e-4, "w16_tile": 4e-4, "fp16": 1.5e-3, "bf16": 8e-3}
