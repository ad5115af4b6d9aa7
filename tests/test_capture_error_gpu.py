"""A Python exception (not a GPU fault) raised inside a CAPTURING step: the error itself surfaces, no graph and no
stream in capture state is left behind, the step's feeds are not lost, and the model goes on -- eager or captured
again, then replayed -- exactly as an undisturbed twin does, bit for bit.

Both injections raise on the capture's own stream before the K7 sort branch is forked onto its side stream, so
ending the capture succeeds and every stream leaves capture state; nothing executes while a capture records, so the
failed step has not touched a table."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


class _Once(object):
    """Wraps a callable: raises RuntimeError("injected") on the first call after arm(), else passes through."""

    def __init__(self, fn):
        self.fn, self.armed, self.fired = fn, False, 0

    def arm(self):
        self.armed = True

    def __call__(self, *a, **k):
        if self.armed:
            self.armed = False
            self.fired += 1
            raise RuntimeError("injected")
        return self.fn(*a, **k)


def test_sharded_step_survives_python_error_in_capture(dev):
    """World-1 ShardedHMF with graph segments.  be.gather_rows_multi -- the step's first launch behind the feed, ahead
    of the K7 fork -- raises once on the capturing (second) step.  Afterwards: same batch again (eager), capture,
    replays; losses and tables equal the twin's, which saw every batch once."""
    import torch
    import torch.distributed as dist
    from arx.dist import ShardedHMF
    from arx.utils.synthetic import SyntheticHMF
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = "29893"
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        n_users, n_items, d, B, S = 300, 400, 64, 32, 128
        syn = SyntheticHMF(n_users=n_users, n_items=n_items, seed=1, permute_logits=False, n_pos=8)
        params = syn.glorot_params(d, seed=2, scale=0.5)
        tables = {'user': params['userembed_cat_0'][2:], 'item': params['itemembed_cat_0'][2:],
                  'item_bias': params['item_bias_cat_0'][2:]}
        ptr = np.concatenate([syn.pos_ptr[:n_users + 1], [syn.pos_ptr[n_users]]]).astype(np.int32)
        rng = np.random.default_rng(3)
        pool = syn.sample_pool(S, rng)
        batches = [syn.sample_batch(B, rng) for _ in range(6)]
        twin, model = [ShardedHMF(n_users, n_items, d, B, S, 0.5, 0, 1, dev, tables=tables, graphs=True)
                       for _ in range(2)]
        for m in (twin, model):
            assert m.use_graphs
            m.set_positives(ptr, syn.pos_items)
            m.set_pool(pool)

        def run(m, batch):
            m.step(*batch)
            return float(m.read_loss().item())

        want = [run(twin, b) for b in batches]
        assert twin.n_captures == 1 and twin.n_replays == 4
        got = [run(model, batches[0])]                              # eager
        hook = model.be.gather_rows_multi = _Once(model.be.gather_rows_multi)
        hook.arm()
        with pytest.raises(RuntimeError) as err:
            model.step(*batches[1])                                 # the capturing step
        assert err.value.args == ("injected",) and hook.fired == 1
        assert model._graphs == {} and model._graph_key is None
        for s_ in (model.stream, model._side):
            if s_ is not None:
                with torch.cuda.stream(s_):
                    assert not torch.cuda.is_current_stream_capturing()
        del model.be.gather_rows_multi                              # (the instance attribute: the method is back)
        got += [run(model, b) for b in batches[1:]]                 # eager, capture, three replays
        assert model.n_captures == 1 and model.n_replays == 3
        assert got == want
        for name in ('E_user', 'A_user', 'E_item', 'A_item', 'b_item', 'Ab_item'):
            assert torch.equal(getattr(model, name), getattr(twin, name)), name
    finally:
        dist.destroy_process_group()


def test_plan_step_survives_python_error_in_capture(dev):
    """LatentProductModel (the shapes of test_graph_lifetime_gpu.py).  The first node the train plan runs forward
    raises once during the capturing Plan.run.  The plan keeps no graph, the feeds taken for the graph are back in
    front of rt.pending_feeds; the retried step (captured now) and the replays behind it equal the twin's."""
    import torch
    from arx.hmf.hmf_model import LatentProductModel
    from arx.utils.synthetic import SyntheticHMF
    d, B, S = 64, 32, 128
    syn = SyntheticHMF(n_users=300, n_items=400, item_mulhot=True, mulhot_vocab=100, avg_len=5, max_len=12, seed=0)
    params = syn.glorot_params(d, seed=1, scale=0.5)
    rng = np.random.default_rng(0)
    pool = syn.sample_pool(S, rng)
    id2idx = {int(v): i for i, v in enumerate(pool)}
    batches = [syn.sample_batch(B, rng) for _ in range(6)]
    pos = syn.positives_dict()

    def make():
        m = LatentProductModel(syn.n_users, syn.n_items, d, 1, B, 0.5, 1.0, syn.u_attr, syn.i_attr,
                               syn.item_ind2logit_ind_dict(), syn.logit_ind2item_ind, loss_function='mw', n_sampled=S,
                               params=params)
        m.prepare_warp(pos, pos)
        return m

    def run(m, k):
        u, i = batches[k]
        return m.step(None, list(u), list(i), None, pool if k == 0 else None, id2idx, loss='mw')

    twin, model = make(), make()
    want = [run(twin, k) for k in range(len(batches))]
    assert twin._plan('train').graph is not None
    got = [run(model, 0)]                                           # eager
    plan, rt = model._plan('train'), model.rt
    assert plan.warm == 1 and plan.graph is None
    pregathered = set(id(n) for _gs, grp in plan._pregather for n in grp)
    node = next(n for n in plan.order if id(n) not in pregathered)
    hook = node.forward = _Once(node.forward)
    taken = []
    take = rt.take_feeds
    rt.take_feeds = lambda: (taken.append(take()), taken[-1])[1]
    hook.arm()
    with pytest.raises(RuntimeError) as err:
        run(model, 1)                                               # the capturing step
    assert err.value.args == ("injected",) and hook.fired == 1
    assert plan.graph is None
    assert len(taken) == 1 and len(taken[0]) > 0
    ids = lambda feeds: [(id(s_), id(d_)) for s_, d_ in feeds]
    assert ids(rt.pending_feeds[:len(taken[0])]) == ids(taken[0])
    assert not torch.cuda.is_current_stream_capturing()
    if plan._k7_stream is not None:
        with torch.cuda.stream(plan._k7_stream):
            assert not torch.cuda.is_current_stream_capturing()
    del node.forward, rt.take_feeds
    got += [run(model, k) for k in range(1, len(batches))]          # capture, replays
    assert plan.graph is not None and plan.graph.feed_groups
    assert got == want
    for name, t in twin.att_emb.tables.items():
        assert torch.equal(model.att_emb.tables[name].E, t.E), name
        assert torch.equal(model.att_emb.tables[name].acc, t.acc), name
