"""The K7 chooser (arx.graph.Plan._choose_fused) without a device: which tables share the fused one-hot pass and
which bag table rides on it.  Stub tables and sites (types.SimpleNamespace, CPU tensors); the expected results are
literals worked out by hand from the conditions the planner carried before the chooser had a name:

    a table joins the candidates with its live sites unless one is a 'window' site, has a column offset, or the
        sites are a bag table of their own: all 'mulhot' on one value array and arena, 8192 < padded slots < 2^31 - 1
    one candidate without multi-hot sites: fused only if a bag table rides on it (real or virtual)
    two or more: group = those of the first one's width, arena and bias arena; padded entries > 1 << 19 -> only the
        tables without multi-hot sites stay; fused if
            (a table with more than 8192 contributions, or union <= 8192 and no multi-hot site)
            and 2 <= tables <= 4 and one-hot sites <= 8 and multi-hot sites <= 8
            and (rows - 1).bit_length() + 2 <= 30 and union <= 1 << 22
    rider (only for a group without multi-hot sites): a bag table (above) with as many live sites as a member, of
        its width, whose sites pair up with the member's on id tensor, row base, coefficient, arena and bias arena,
        the member's entity -> row map being one-to-one -> real, index = the member's; that member moves to the front.
        Else the first bag table of the group's width and arenas with group <= 3 tables, one-hot + bag sites <= 8,
        entities.bit_length() + 2 <= 30 -> virtual, index None.
"""
import types

import pytest
import torch

from arx import graph as G

NS = types.SimpleNamespace


class _World(object):
    """Stub tables over one or more gradient arenas; lookups (id tensors) are shared by name."""

    def __init__(self):
        self.tables = []
        self.arenas = {}
        self.ids = {}

    def _node(self, arena, row0):
        a = self.arenas.setdefault(arena, (object(), object()))
        return NS(_grad_written=True, bias_grad_used=False, arena=a[0], arena_b=a[1], row0=row0)

    def _ids(self, name, n):
        if name not in self.ids:
            self.ids[name] = NS(value=torch.zeros(n, dtype=torch.int32))
        return self.ids[name]

    def table(self, rows, d=32):
        return NS(E=torch.empty(rows, d), acc=None, bias=None, bias_acc=None)

    def onehot(self, rows, lookups, d=32, arena='a', cmap=None, kind='cat'):
        """lookups: [(ids name, n, row base)]"""
        t = self.table(rows, d)
        sites = [NS(table=t, kind=kind, col_off=0, cap=n, n=n, maps=(cmap,), ids_node=self._ids(name, n),
                    node=self._node(arena, r0), coef=1.0, max_len=1) for name, n, r0 in lookups]
        self.tables.append(G.TableEntry(t, sites, {}, sum(s.cap for s in sites)))
        return self.tables[-1]

    def bags(self, rows, entities, lookups, max_len, d=32, arena='a', own_maps=False):
        t = self.table(rows, d)

        def maps():
            return (torch.zeros(entities * max_len, dtype=torch.int32),
                    torch.arange(entities, dtype=torch.int32) * max_len,
                    torch.full((entities,), max_len, dtype=torch.int32))
        shared = maps()
        sites = [NS(table=t, kind='mulhot', col_off=0, cap=n * max_len, n=n, maps=maps() if own_maps else shared,
                    ids_node=self._ids(name, n), node=self._node(arena, r0), coef=1.0, max_len=max_len)
                 for name, n, r0 in lookups]
        self.tables.append(G.TableEntry(t, sites, {}, sum(s.cap for s in sites)))
        return self.tables[-1]

    def choose(self):
        plan = G.Plan.__new__(G.Plan)             # the chooser reads the tables and its own cache, nothing else
        plan.tables, plan._rider_cache = self.tables, {}
        group, rider = plan._choose_fused()
        return [m.entry for m in group], rider


def _two(n_a, n_b, **kw_b):
    w = _World()
    a = w.onehot(1000, [('u', n_a, 0)])
    b = w.onehot(2000, [('i', n_b, n_a)], **kw_b)
    return w, a, b


@pytest.mark.parametrize("n_a, n_b, fused", [
    (64, 64, True),              # union 128 <= 8192: one rank-sort chain for both
    (4096, 5000, False),         # no table above 8192, union 9096 above it
    (16384, 1024, True),         # a table above 8192
    (8192, 1, False),            # exactly 8192 is not above; union 8193
    (4096, 4096, True),          # union exactly 8192
])
def test_two_onehot_tables(n_a, n_b, fused):
    w, a, b = _two(n_a, n_b)
    group, rider = w.choose()
    assert rider is None
    assert group == ([a, b] if fused else [])


def test_other_width_or_arena_leaves_the_group():
    for kw in (dict(d=64), dict(arena='b')):
        w, a, b = _two(64, 64, **kw)
        c = w.onehot(500, [('p', 32, 128)])
        group, rider = w.choose()
        assert group == [a, c] and rider is None
        w, a, b = _two(64, 64, **kw)          # ... and with two tables only, nothing is left to share a pass
        assert w.choose() == ([], None)


def test_padded_segments_past_half_a_million_leave():
    w, a, b = _two(16384, 1024)
    # two multi-hot features over different value arrays are no bag table of their own (_bags_ok: one value array),
    # so their table is a candidate with pre-expanded segments: 2 * 40000 * 8 = 640000 padded entries > 1 << 19
    m = w.bags(300, 100, [('m0', 40000, 20000), ('m1', 40000, 60000)], max_len=8, own_maps=True)
    group, rider = w.choose()
    assert group == [a, b] and rider is None
    w, a, b = _two(16384, 1024)               # ... 2 * 30000 * 8 = 480000 stay
    m = w.bags(300, 100, [('m0', 30000, 20000), ('m1', 30000, 50000)], max_len=8, own_maps=True)
    group, rider = w.choose()
    assert group == [a, b, m] and rider is None


def test_multihot_segments_join_below_the_limits():
    w, a, b = _two(16384, 1024)
    m = w.bags(300, 100, [('m', 1000, 20000)], max_len=8)       # 8000 padded slots <= 8192: no pass of its own
    group, rider = w.choose()
    assert group == [a, b, m] and rider is None
    w, a, b = _two(64, 64)                                        # ... but the small union shares only without them
    w.bags(300, 100, [('m', 100, 128)], max_len=8)
    assert w.choose() == ([], None)


def test_row_count_needs_too_many_key_bits():
    w = _World()
    big = NS(E=NS(shape=((1 << 28) + 1, 32)), acc=None, bias=None, bias_acc=None)   # (2^28).bit_length() + 2 == 31
    a = w.onehot(1000, [('u', 64, 0)])
    b = w.onehot(2000, [('i', 64, 64)])
    w.tables[1] = b._replace(table=big)
    assert w.choose() == ([], None)
    ok = NS(E=NS(shape=(1 << 28, 32)), acc=None, bias=None, bias_acc=None)      # (2^28 - 1).bit_length() + 2 == 30
    w.tables[1] = b._replace(table=ok)
    group, rider = w.choose()
    assert len(group) == 2 and rider is None


def _het(bag_ids=('i', 't'), bag_lookups=None, cmap=None, max_len=9):
    """users [1024], items: targets [1024] + pool [128] one-hot; a bag table over the items."""
    w = _World()
    u = w.onehot(1000, [('u', 1024, 0)])
    i = w.onehot(2000, [('i', 1024, 1024), ('t', 128, 2048)], cmap=cmap)
    b = w.bags(300, 2000, bag_lookups or [(bag_ids[0], 1024, 1024), (bag_ids[1], 128, 2048)], max_len=max_len)
    return w, u, i, b


def test_real_rider_moves_its_table_to_the_front():
    w, u, i, b = _het()                        # (1024 + 128) * 9 = 10368 padded slots > 8192
    group, rider = w.choose()
    assert group == [i, u]
    assert rider.entry is b and rider.index == 1 and rider.virtual is False and rider.use_bias is False
    assert rider.live == b.sites
    assert tuple(rider)[:4] == (b, b.sites, False, False)


def test_other_id_tensors_make_the_rider_virtual():
    w, u, i, b = _het(bag_ids=('x', 'y'))
    group, rider = w.choose()
    assert group == [u, i]
    assert rider.entry is b and rider.index is None and rider.virtual is True


def test_small_bag_table_is_no_rider():
    w, u, i, b = _het(max_len=7)               # 1152 * 7 = 8064 <= 8192: joins as padded segments
    group, rider = w.choose()
    assert rider is None and group == []       # union 2176 + 8064 > 8192 with a multi-hot site, no table above 8192
    w, u, i, b = _het(bag_lookups=[('i', 1024, 1024)], max_len=8)      # exactly 8192
    assert w.choose()[1] is None


def test_lone_onehot_table():
    w = _World()
    w.onehot(1000, [('u', 20000, 0)])
    assert w.choose() == ([], None)            # keeps its own pass
    b = w.bags(300, 1000, [('u', 20000, 0)], max_len=4)
    group, rider = w.choose()                  # ... unless a bag table rides on it
    assert len(group) == 1 and rider.entry is b and rider.index == 0 and not rider.virtual


def test_window_site_keeps_its_table_out():
    w, a, b = _two(64, 64)
    c = w.onehot(500, [('c', 32, 128)])
    w.onehot(2000, [('w', 256, 160)], kind='window')
    group, rider = w.choose()
    assert group == [a, b, c] and rider is None


def test_sites_without_gradient_do_not_count():
    w, a, b = _two(64, 64)
    b.sites[0].node._grad_written = False
    assert w.choose() == ([], None)


def test_non_injective_row_map_rejects_the_real_rider():
    cmap = torch.arange(2000, dtype=torch.int32)
    w, u, i, b = _het(cmap=cmap.clone())
    assert w.choose()[1].virtual is False
    cmap[5] = 4                                # two entities on one row
    w, u, i, b = _het(cmap=cmap)
    group, rider = w.choose()
    assert group == [u, i] and rider.virtual is True and rider.index is None


def test_rider_bias_flag_follows_the_backward():
    w, u, i, b = _het()
    b.table.bias = torch.zeros(300)
    assert w.choose()[1].use_bias is False
    b.sites[1].node.bias_grad_used = True
    assert w.choose()[1].use_bias is True
