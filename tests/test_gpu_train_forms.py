"""The forms of the one AdamW kernel and the one gather kernel of csrc/train.hip agree bit for bit: the four fused_adamw* operators
differ only in where the per-step inputs come from, mv_multi_gather / mv_multi_gather_acc only in `=` against `+=`."""
from ctypes import c_void_p

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HP = (1e-2, 0.8, 0.99, 1e-8, 1e-1)          # lr, beta1, beta2, eps, weight_decay
GS = 0.5


@pytest.fixture(scope="module")
def ns():
    from hifigan_modified import _native
    _native.lib()
    assert torch.cuda.is_available(), "GPU tests need cuda:0"
    return torch.ops.mi355x_vocoder


def _bits(t):
    return t.view(torch.int32)


# 1 048 583 = one full grid of 4096 x 256 threads + 7: the grid-stride loop runs a second, partial pass
@pytest.mark.parametrize("n", [1, 7, 4099, 65537, 1048583])
def test_adamw_forms_bit_identical(ns, n):
    g = torch.Generator().manual_seed(n)
    state0 = [torch.randn(n, generator=g).cuda(), torch.randn(n, generator=g).cuda() * 0.1, torch.rand(n, generator=g).cuda() * 0.1]
    grads = [torch.randn(n, generator=g).cuda() for _ in range(3)]
    forms = {k: [t.clone() for t in state0] for k in ("value", "clip_value", "hp", "clip_dev", "dev")}     # each: p, m, v
    hp = torch.tensor(HP, dtype=torch.float32, device="cuda")
    one = torch.ones(1, dtype=torch.float32, device="cuda")
    for t, gr in enumerate(grads, start=1):
        step = torch.tensor([t], dtype=torch.int32, device="cuda")
        arena = lambda k: (forms[k][0], gr, forms[k][1], forms[k][2])
        ns.fused_adamw_(*arena("value"), *HP, t, GS)
        ns.fused_adamw_clip_(*arena("clip_value"), None, None, *HP, t, GS, one)
        ns.fused_adamw_hp_(*arena("hp"), hp, step, GS)
        ns.fused_adamw_clip_(*arena("clip_dev"), hp, step, 0.0, 0.0, 0.0, 0.0, 0.0, 0, GS, one)
        ns.fused_adamw_dev_(*arena("dev"), *HP, step, GS)
        for a, b in (("clip_value", "value"), ("clip_dev", "hp"), ("hp", "dev")):
            for x, y, what in zip(forms[a], forms[b], "pmv"):
                assert torch.equal(_bits(x), _bits(y)), (a, b, what, t)
    assert not torch.equal(forms["value"][0], state0[0]) and bool(torch.isfinite(forms["value"][0]).all())   # (the steps did move p)


SENTINEL = -7.5


# 16384 is the gather's chunk: one block column at 16384, a second one for the last element at 16385
@pytest.mark.parametrize("n", [1, 7, 16384, 16385])
def test_gather_forms(ns, n):
    from hifigan_modified import _native as N
    from hifigan_modified import ops
    from hifigan_modified.optim import _DESC
    g = torch.Generator().manual_seed(n)
    srcs = [torch.randn(n, generator=g).cuda(), torch.randn(n, generator=g).cuda().bfloat16(), None,
            torch.randn(n, generator=g).cuda().half()]
    stride = (n + 7) // 8 * 8 + 8                           # at least 8 padding words behind every parameter
    offsets = [8 + i * stride for i in range(len(srcs))]    # and 8 in front of the first
    total = offsets[-1] + stride
    d = np.zeros(len(srcs), dtype=_DESC)
    d["dst_off"], d["n"] = offsets, n
    for i, s in enumerate(srcs):
        if s is not None:
            d["src"][i], d["dtype"][i] = s.data_ptr(), ops._DT[s.dtype]
    table = torch.from_numpy(d.view(np.uint8).reshape(-1).copy()).cuda()
    pad = torch.ones(total, dtype=torch.bool, device="cuda")
    for o in offsets:
        pad[o:o + n] = False

    def region(flat, i):
        return flat[offsets[i]:offsets[i] + n]

    # plain form on a buffer full of the sentinel: sources widened exactly, zeros for the NULL source, padding untouched
    plain = torch.full((total,), SENTINEL, device="cuda")
    N.call("mv_multi_gather", c_void_p(table.data_ptr()), len(srcs), n, c_void_p(plain.data_ptr()), ops._stream())
    for i, s in enumerate(srcs):
        want = torch.zeros(n, device="cuda") if s is None else s.float()
        assert torch.equal(_bits(region(plain, i)), _bits(want)), i
    assert bool((plain[pad] == SENTINEL).all())
    # zero_ + the accumulating form = the plain form's bits; the sentinel, put back into the padding after zero_, survives
    acc = torch.full((total,), SENTINEL, device="cuda")
    ns.zero_(acc)
    assert float(acc.abs().max()) == 0.0
    acc[pad] = SENTINEL
    ns.multi_gather_acc_(table, len(srcs), n, acc)
    assert torch.equal(_bits(acc), _bits(plain))
    # the accumulating form on the sentinel itself: one fp32 add per element, the NULL source's words and the padding left alone
    acc = torch.full((total,), SENTINEL, device="cuda")
    ns.multi_gather_acc_(table, len(srcs), n, acc)
    for i, s in enumerate(srcs):
        want = torch.full((n,), SENTINEL, device="cuda") if s is None else s.float() + SENTINEL
        assert torch.equal(_bits(region(acc, i)), _bits(want)), i
    assert bool((acc[pad] == SENTINEL).all())
