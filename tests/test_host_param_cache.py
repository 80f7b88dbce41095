"""ops.DerivedCache / ops.param_state on CPU tensors (no GPU, no native library): the one staleness rule behind every cached
cast and packed weight.  The builder only counts its calls."""
import gc

import torch

import conftest  # noqa: F401  (puts the package on sys.path)
from hifigan_modified import ops


class _Builder:
    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return ["value", self.calls]


class _Owner:
    """What the cache needs of a flat-arena optimizer."""

    def __init__(self, params):
        self.params = list(params)
        ops.register_shadow_owner(self, self.params)

    def owns(self, p):
        return any(q is p for q in self.params)


def _param(n=4):
    return torch.nn.Parameter(torch.arange(float(n)))


def test_unchanged_parameter_hits_and_returns_the_same_object():
    c, b, p = ops.DerivedCache(), _Builder(), _param()
    v1 = c.lookup(p, "cast", b)
    v2 = c.lookup(p, "cast", b)
    assert b.calls == 1 and v2 is v1
    assert c.lookup(p, "other tag", b) is not v1 and b.calls == 2      # tags do not alias


def test_in_place_update_misses():
    c, b, p = ops.DerivedCache(), _Builder(), _param()
    v1 = c.lookup(p, 0, b)
    with torch.no_grad():
        p.add_(1)
    v2 = c.lookup(p, 0, b)
    assert b.calls == 2 and v2 is not v1
    assert c.lookup(p, 0, b) is v2 and b.calls == 2


def test_data_reassignment_misses():
    c, b, p = ops.DerivedCache(), _Builder(), _param()
    c.lookup(p, 0, b)
    version = p._version
    p.data = torch.zeros(4)                                  # new storage, same tensor object, same version
    assert p._version == version
    c.lookup(p, 0, b)
    assert b.calls == 2
    c.lookup(p, 0, b)
    assert b.calls == 2


def test_unattributed_bump_makes_every_entry_miss_once():
    c, b = ops.DerivedCache(), _Builder()
    ps = [_param() for _ in range(3)]
    owner = _Owner(ps[:1])                                   # owned or not: an unattributed bump drops it
    for p in ps:
        c.lookup(p, 0, b)
    ops.bump_param_epoch()
    for p in ps:
        c.lookup(p, 0, b)
    assert b.calls == 6
    for p in ps:
        c.lookup(p, 0, b)
    assert b.calls == 6
    del owner


def test_attributed_bump_drops_only_the_owners_parameters():
    c, b = ops.DerivedCache(), _Builder()
    pa, pb, free = [_param(), _param()], [_param()], _param()
    owner_a, owner_b = _Owner(pa), _Owner(pb)
    for p in pa + pb + [free]:
        c.lookup(p, 0, b)
    assert b.calls == 4
    ops.bump_param_epoch(owner_a)
    for p in pb:
        c.lookup(p, 0, b)
    assert b.calls == 4                                      # b's parameters hit
    for p in pa:
        c.lookup(p, 0, b)
    assert b.calls == 6                                      # a's miss
    c.lookup(free, 0, b)
    assert b.calls == 7                                      # no owner: any bump may have touched it
    for p in pa + pb + [free]:
        c.lookup(p, 0, b)
    assert b.calls == 7
    del owner_a, owner_b


def test_dead_parameter_entry_is_never_returned_and_is_pruned():
    c, b = ops.DerivedCache(prune_at=2), _Builder()
    p = _param()
    dead_value = c.lookup(p, 0, b)
    (key, (refs, state, _)), = c.d.items()
    del p
    gc.collect()
    assert refs[0]() is None
    q = _param()                                             # same shape, same version; CPython may even recycle the id
    # force the id collision: the dead tensor's entry under q's key, with q's current state
    del c.d[key]
    c.d[((id(q),), 0)] = (refs, ops.param_state(q), dead_value)
    v = c.lookup(q, 0, b)
    assert v is not dead_value and b.calls == 2
    # pruning: dead entries go when the table grows past its threshold
    r = _param()
    c.lookup(r, 0, b)
    c.lookup(r, 1, b)
    del r
    gc.collect()
    assert len(c.d) == 3
    s = _param()
    c.lookup(s, 0, b)                                        # len 3 > 2: the store prunes r's two entries first
    assert len(c.d) == 2 and all(ref() is not None for e in c.d.values() for ref in e[0])


def test_multi_parameter_key_misses_when_any_member_changes():
    c, b = ops.DerivedCache(), _Builder()
    ps = tuple(_param() for _ in range(3))
    v = c.lookup(ps, "pack", b)
    assert c.lookup(ps, "pack", b) is v and b.calls == 1
    for i, p in enumerate(ps):
        with torch.no_grad():
            p.mul_(2)
        c.lookup(ps, "pack", b)
        assert b.calls == 2 + i
        c.lookup(ps, "pack", b)
        assert b.calls == 2 + i
    ps[1].data = torch.ones(4)
    c.lookup(ps, "pack", b)
    assert b.calls == 5
    assert c.lookup((ps[0], ps[2], ps[1]), "pack", b) is not None and b.calls == 6      # another tuple is another key


def test_param_state_components():
    p = _param()
    (s0,) = ops.param_state(p)
    assert s0 == (p._version, p.data_ptr(), p.device, ops.param_epoch_of(p))
    assert ops.param_state(p, p) == (s0, s0)


def test_mark_current_adopts_the_parameters_present_state():
    c, b, p = ops.DerivedCache(), _Builder(), _param()
    v = c.lookup(p, 0, b)
    with torch.no_grad():
        p.add_(1)
    (key,) = c.d
    c.mark_current(key)                                      # (what a batched re-pack does after rewriting the value in place)
    assert c.lookup(p, 0, b) is v and b.calls == 1
