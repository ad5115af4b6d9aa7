"""The row-sharded skip-gram / CBOW recommender (arx.dist.ShardedW2V) without a GPU: gloo ranks over the numpy compute
double (tests/numpy_backend_w2v.py) against tests/w2v_sampled_ref.py::RefW2VSampled on the GLOBAL batch in fp64.

  training   worlds 2 and 3, CBOW / skip-gram x 'mw' / 'mce', n_input = 3, five steps with pool changes: the loss of
             every step, and every row and Adagrad slot of the three tables after the last.  The batches hold an item
             twice in one window, a context item asked for from two ranks, an item that is context of one row, target
             of another and in the pool, a duplicate user, and one step whose context items all live on rank 0
  n_input=1  CBOW and skip-gram are the same model
  serving    recommend (with and without exclude_seen) and evaluate ('warp', 'ce') at world 2 against numpy on the
             gathered tables with x_test of the FULL window, for a skip-gram model too
  checkpoints   saved at world 2, restored at world 3, one more step
  the constructor's and the route's refusals, and the argument checks of the two kernels (no device is touched)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "a-recsys_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

N_USERS, N_ITEMS, D, B_LOC, S, N_IN, LR = 60, 90, 16, 8, 16, 3, 0.5
W2V_SEED = 5           # ('mw': no hinge argument of any step within 1e-4 of the kink, asserted below on the reference)
NAMES = ('userembed_cat_0', 'itemembed_cat_0', 'item_outputembed_cat_0', 'item_output_bias_cat_0')


def _init(rank, world, port):
    for p in (ROOT, os.path.join(ROOT, "a-recsys_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    return dist


def w2v_world(n_users=N_USERS, n_items=N_ITEMS, d=D):
    from arx.utils.synthetic import SyntheticHMF
    syn = SyntheticHMF(n_users=n_users, n_items=n_items, seed=1, permute_logits=False, n_pos=6)
    syn.u_attr.set_model_size(d)
    syn.i_attr.set_model_size(d)
    params = syn.glorot_params(d, seed=2, item_output=True, scale=0.5)
    return syn, params, {k: params[k][2:] for k in NAMES}


def w2v_ref(syn, params, cbow, loss, B, d=D, n_sampled=S, n_in=N_IN, lr=LR):
    from w2v_sampled_ref import RefW2VSampled
    ref = RefW2VSampled('cbow' if cbow else 'skipgram', d, B, lr, syn.u_attr, syn.i_attr,
                        syn.item_ind2logit_ind_dict(), syn.logit_ind2item_ind, n_sampled, n_input_items=n_in,
                        loss_function=loss, use_sep_item=True, params={k: v.copy() for k, v in params.items()})
    pos = syn.positives_dict()
    ref.prepare_warp(pos, pos)
    return ref


def set_positives(model, syn, rank, world):
    own = np.arange(rank, syn.n_users, world)
    ptr, items = np.zeros(len(own) + 2, dtype=np.int32), []
    for k, u in enumerate(own):
        items.extend(syn.pos_items[syn.pos_ptr[u]:syn.pos_ptr[u + 1]].tolist())
        ptr[k + 1] = len(items)
    ptr[-1] = ptr[-2]
    model.set_positives(ptr, np.asarray(items, dtype=np.int32))


def w2v_batches(syn, world, seed, n_steps=5, b_loc=B_LOC, n_sampled=S, n_in=N_IN):
    """Per step (pool or None, [users], [targets], [context [n_in, b_loc]]) of every rank.  The pool changes at steps
    0, 2 (every slot on the last owner) and 4 (three quarters on owner 0).  Every step: a duplicate user on rank 0, an
    item twice in one window, the context item (t = 0) of a row of rank 0 asked for by the last rank too.  Every step
    but 3: the first pool item is the t = 0 context of a row of rank 0 and the target of a row of the last rank.
    Step 3: every context item lives on rank 0."""
    n_users, n_items = syn.n_users, syn.n_items
    rng = np.random.default_rng(seed)
    out, cur = [], None
    for step in range(n_steps):
        pool = None
        if step % 2 == 0:
            if step == 0:
                pool = rng.choice(n_items, size=n_sampled, replace=False)
            elif step == 2:
                pool = rng.choice(np.arange(world - 1, n_items, world), size=n_sampled, replace=False)
            else:
                hot = rng.choice(np.arange(0, n_items, world), size=(3 * n_sampled) // 4, replace=False)
                rest = rng.choice(np.setdiff1d(np.arange(n_items), hot), size=n_sampled - len(hot), replace=False)
                pool = rng.permutation(np.concatenate([hot, rest]))
            cur = pool = pool.astype(np.int32)
        gu, gi, gc = [], [], []
        for g in range(world):
            users = rng.integers(0, len(np.arange(g, n_users, world)), size=b_loc) * world + g
            gu.append(users)
            gi.append(syn.pos_items[syn.pos_ptr[users] + rng.integers(0, syn.n_pos, size=b_loc)].astype(np.int64))
            if step == 3:
                gc.append(rng.integers(0, n_items // world, size=(n_in, b_loc)) * world)
            else:
                gc.append(rng.integers(0, n_items, size=(n_in, b_loc)))
        gu[0][1] = gu[0][0]
        for g in range(world):
            gc[g][n_in - 1][3] = gc[g][0][3]
        if step != 3:
            gc[0][0][6] = cur[0]
            gi[world - 1][7] = cur[0]
        gc[world - 1][0][4] = gc[0][0][5]
        out.append((pool, gu, gi, gc))
    return out


def check_batches(world, batches, n_in=N_IN):
    cur = None
    for step, (pool, gu, gi, gc) in enumerate(batches):
        cur = pool if pool is not None else cur
        assert gu[0][1] == gu[0][0]                                           # a duplicate user
        assert all(gc[g][n_in - 1][3] == gc[g][0][3] for g in range(world)) or n_in == 1   # twice in one window
        assert gc[world - 1][0][4] == gc[0][0][5]                             # one context item, two ranks
        if step != 3:                                                         # context, target and pool at once
            assert gc[0][0][6] == cur[0] and gi[world - 1][7] == cur[0] and cur[0] in set(cur.tolist())
    assert all((c % world == 0).all() for c in batches[3][3])                 # step 3: all context rows on rank 0


def hinge_gap(ref, users, ctx, targets):
    """min |x_s - t + 1| over the pool logits of the batch at the reference's current tables (masked entries too)."""
    x_train = ref._x(users, ctx)[0]
    logits = ref.att_emb.get_prediction(x_train, 'sampled', 1)[0]
    t = ref.att_emb.get_target_score(x_train, targets)[0]
    return float(np.abs(np.asarray(logits) - np.asarray(t).reshape(-1, 1) + 1.0).min())


def ref_step(ref, pool, gu, gi, gc, check_kink):
    users, targets = np.concatenate(gu).tolist(), np.concatenate(gi).tolist()
    ctx = np.concatenate(gc, axis=1).tolist()
    id2idx = {int(v): i for i, v in enumerate(pool)} if pool is not None else None
    if pool is not None:
        ref.stage_pool(pool, id2idx)
    if check_kink:
        gap = hinge_gap(ref, users, ctx, targets)
        assert gap > 1e-4, gap
    return float(ref.step(users, ctx, targets))


def compare_tables(got, ref, rtol=1e-4, atol=1e-6):
    P, A = ref.att_emb.params, ref.att_emb.slots
    for name in NAMES:
        for suffix, src in (('', P), ('/Adagrad', A)):
            want = src[name][2:]
            np.testing.assert_allclose(got[name + suffix].reshape(want.shape), want, rtol=rtol, atol=atol,
                                       err_msg=name + suffix)


@pytest.mark.parametrize("cbow", [True, False], ids=['cbow', 'skipgram'])
@pytest.mark.parametrize("world", [2, 3])
def test_mw_reference_stays_clear_of_the_kink(world, cbow):
    """fp32 and fp64 may branch differently near x - t + 1 = 0: on the fp64 reference no pool logit of any step of
    the training test lies within 1e-4 of it (the seed is chosen so; nothing is left out)."""
    syn, params, _ = w2v_world()
    batches = w2v_batches(syn, world, W2V_SEED)
    check_batches(world, batches)
    ref = w2v_ref(syn, params, cbow, 'mw', B_LOC * world)
    for pool, gu, gi, gc in batches:
        ref_step(ref, pool, gu, gi, gc, True)


def _model(rank, world, tables, cbow, loss, n_in=N_IN, **kw):
    from arx.dist import ShardedW2V
    from numpy_backend_w2v import NumpyW2VBackend
    return ShardedW2V(N_USERS, N_ITEMS, D, B_LOC, S, n_in, LR, rank, world, 'cpu', cbow=cbow, loss=loss,
                      tables=tables, backend=NumpyW2VBackend(), **kw)


def _train_worker(rank, world, port, out_dir, cbow, loss):
    dist = _init(rank, world, port)
    syn, params, tables = w2v_world()
    model = _model(rank, world, tables, cbow, loss)
    set_positives(model, syn, rank, world)
    ref = w2v_ref(syn, params, cbow, loss, B_LOC * world)
    batches = w2v_batches(syn, world, W2V_SEED)
    check_batches(world, batches)
    grew = after_growth = padded = False
    n_train = N_IN if cbow else 1
    for step, (pool, gu, gi, gc) in enumerate(batches):
        l_ref = ref_step(ref, pool, gu, gi, gc, loss == 'mw')
        if pool is not None:
            model.set_pool(pool)
        cap_c0 = model.cap_c
        route = model.prepare_route(gu[rank], gi[rank], gc[rank])
        req = np.concatenate([c[:n_train].reshape(-1) for c in gc])
        assert route['Rc'] == int((req % world == rank).sum()) and route['n_req'] == n_train * B_LOC
        if step == 3:
            assert route['Rc'] == (world * n_train * B_LOC if rank == 0 else 0)
        model.step(route)
        l_got = float(model.read_loss().item())
        assert abs(l_got - l_ref) <= 1e-5 * abs(l_ref), (step, l_got, l_ref)
        after_growth |= grew
        grew |= model.cap_c > cap_c0
        padded |= route['Rc'] < model.cap_c
    if rank == 0:
        assert grew and after_growth, "rank 0's context capacity did not grow mid-run"
    assert padded
    compare_tables(model.gather_global_tables(slots=True), ref)
    with open(os.path.join(out_dir, "ok%d" % rank), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


CONFIGS = [(w, c, l) for w in (2, 3) for c in (True, False) for l in ('mw', 'mce')]


@pytest.mark.parametrize("world,cbow,loss", CONFIGS,
                         ids=['w%d-%s-%s' % (w, 'cbow' if c else 'skipgram', l) for w, c, l in CONFIGS])
def test_sharded_w2v_steps_match_fp64_gloo(tmp_path, world, cbow, loss):
    import torch.multiprocessing as mp
    port = 29300 + (os.getpid() % 400) + CONFIGS.index((world, cbow, loss))
    mp.spawn(_train_worker, args=(world, port, str(tmp_path), cbow, loss), nprocs=world, join=True)
    assert all(os.path.exists(tmp_path / ("ok%d" % r)) for r in range(world))


def _n1_worker(rank, world, port, out_dir):
    dist = _init(rank, world, port)
    syn, params, tables = w2v_world()
    models = [_model(rank, world, tables, cbow, 'mw', n_in=1) for cbow in (True, False)]
    for m in models:
        set_positives(m, syn, rank, world)
    for pool, gu, gi, gc in w2v_batches(syn, world, W2V_SEED, n_steps=3, n_in=1):
        for m in models:
            if pool is not None:
                m.set_pool(pool)
            m.step(gu[rank], gi[rank], gc[rank])
    a, b = (m.gather_global_tables(slots=True) for m in models)
    assert set(a) == set(b) and len(a) == 8
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert not np.array_equal(a['itemembed_cat_0'], tables['itemembed_cat_0'])        # (it did train)
    with open(os.path.join(out_dir, "ok%d" % rank), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


def test_n_input_1_cbow_and_skipgram_are_one_model_gloo(tmp_path):
    import torch.multiprocessing as mp
    port = 29320 + (os.getpid() % 400)
    mp.spawn(_n1_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert all(os.path.exists(tmp_path / ("ok%d" % r)) for r in range(2))


# ---------------------------------------------------------------------------------------------------------- serving
def x_test(T, users, ctx):
    """0.5 u + (0.5 / n) sum_t C[ctx_t] over the full window, fp64; ctx [n, m]."""
    U, C = T['userembed_cat_0'].astype(np.float64), T['itemembed_cat_0'].astype(np.float64)
    ctx = np.asarray(ctx, dtype=np.int64).reshape(-1, len(users))
    return 0.5 * U[np.asarray(users, dtype=np.int64)] + (0.5 / ctx.shape[0]) * C[ctx].sum(0)


def scores(T, users, ctx):
    I = T['item_outputembed_cat_0'].astype(np.float64)
    return x_test(T, users, ctx) @ I.T + T['item_output_bias_cat_0'].astype(np.float64).reshape(1, -1)


def topk_ref(x, users, k, ex=None, min_gap=1e-5):
    """ids [m, k] by (score desc, id asc), excluded -> out; asserts that no two of the first k + 1 scores of a row
    are closer than min_gap (fp32 and fp64 then order them alike)."""
    out = np.full((len(users), k), -1, dtype=np.int64)
    for j, u in enumerate(users):
        row = x[j].copy()
        if ex is not None and len(ex.get(int(u), ())):
            row[np.asarray(sorted(set(ex[int(u)])), dtype=np.int64)] = -np.inf
        o = np.lexsort((np.arange(len(row)), -row))
        top = row[o[:k + 1]]
        top = top[np.isfinite(top)]
        assert len(top) < 2 or np.abs(np.diff(top)).min() > min_gap
        o = o[:k]
        out[j] = np.where(np.isneginf(row[o]), -1, o)
    return out


def eval_ref(x, users, items, loss, pos):
    out = []
    for j, (u, i) in enumerate(zip(users, items)):
        row, t = x[j], x[j][i]
        if loss == 'ce':
            m = row.max()
            out.append(m + np.log(np.exp(row - m).sum()) - t)
            continue
        keep = np.ones(len(row), dtype=bool)
        keep[np.asarray(sorted(set(pos.get(int(u), ()))), dtype=np.int64)] = False
        out.append(np.log1p(np.maximum(row - t + 1.0, 0.0)[keep].sum()))
    return np.asarray(out, dtype=np.float64)


def serve_rows(syn, g, world, b_loc=B_LOC, n_in=N_IN):
    """(users, context [n_in, m], targets) of rank g: rank 0 lists a user twice (two contexts), the last rank fewer
    rows than B_loc."""
    rng = np.random.default_rng(300 + g)
    own = np.arange(g, syn.n_users, world)
    users = own[[0, 1, 2, 1]] if g == 0 else own[:b_loc - 3]
    ctx = rng.integers(0, syn.n_items, size=(n_in, len(users)))
    ctx[n_in - 1][0] = ctx[0][0]
    return users, ctx, rng.integers(0, syn.n_items, size=len(users))


def check_serving(model, syn, rank, world, k=7):
    """recommend / evaluate of `model` against numpy on its gathered tables (a collective: every rank calls it)."""
    T = model.gather_global_tables()
    rows = [serve_rows(syn, g, world, model.B_loc, model.n_input) for g in range(world)]
    users, ctx, items = rows[rank]
    x = scores(T, users, ctx)
    x_all = np.concatenate([scores(T, u, c) for u, c, _ in rows])
    all_u, all_i = np.concatenate([r[0] for r in rows]), np.concatenate([r[2] for r in rows])
    got, vals = model.recommend(users, ctx, k, return_values=True)
    want = topk_ref(x, users, k)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    np.testing.assert_allclose(vals.cpu().numpy(), np.take_along_axis(x, want, 1), rtol=1e-5, atol=1e-6)
    pos = syn.positives_dict()
    own = np.arange(rank, syn.n_users, world)
    model.prepare_recommend_exclusions({int(u): pos[int(u)] for u in own})
    cut = topk_ref(x, users, k, pos)
    np.testing.assert_array_equal(model.recommend(users, ctx, k, exclude_seen=True).cpu().numpy(), cut)
    assert (cut != want).any()                                   # the lists took something out of somebody's top k
    model.prepare_eval_positives({int(u): pos[int(u)][:3] for u in own})
    pos_eval = {u: pos[u][:3] for u in pos}
    for loss in ('warp', 'ce'):
        mean, per_row = model.evaluate(users, ctx, items, loss=loss, return_rows=True)
        np.testing.assert_allclose(per_row.cpu().numpy(), eval_ref(x, users, items, loss, pos_eval), rtol=1e-5)
        np.testing.assert_allclose(mean, eval_ref(x_all, all_u, all_i, loss, pos_eval).mean(), rtol=1e-5)
    with pytest.raises(ValueError, match="context"):
        model.recommend(users, ctx[:-1], k)                      # a window short of n_input rows
    with pytest.raises(ValueError, match="context"):
        model.evaluate(users[:1], np.full((model.n_input, 1), syn.n_items), items[:1], loss='ce')


def _serve_worker(rank, world, port, out_dir, cbow):
    dist = _init(rank, world, port)
    syn, params, tables = w2v_world()
    model = _model(rank, world, tables, cbow, 'mw')
    set_positives(model, syn, rank, world)
    for pool, gu, gi, gc in w2v_batches(syn, world, W2V_SEED, n_steps=2):
        if pool is not None:
            model.set_pool(pool)
        model.step(gu[rank], gi[rank], gc[rank])
    before = model.gather_global_tables(slots=True)
    check_serving(model, syn, rank, world)
    after = model.gather_global_tables(slots=True)
    assert all(np.array_equal(before[k], after[k]) for k in before)           # serving touched no table
    with open(os.path.join(out_dir, "ok%d" % rank), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


@pytest.mark.parametrize("cbow", [True, False], ids=['cbow', 'skipgram'])
def test_sharded_w2v_recommend_and_evaluate_gloo(tmp_path, cbow):
    import torch.multiprocessing as mp
    port = 29340 + (os.getpid() % 400) + int(cbow)
    mp.spawn(_serve_worker, args=(2, port, str(tmp_path), cbow), nprocs=2, join=True)
    assert all(os.path.exists(tmp_path / ("ok%d" % r)) for r in range(2))


# ------------------------------------------------------------------------------------------------------ checkpoints
def _bitwise_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _save_worker(rank, world, port, out_dir):
    dist = _init(rank, world, port)
    syn, params, tables = w2v_world()
    model = _model(rank, world, tables, True, 'mw')
    set_positives(model, syn, rank, world)
    for pool, gu, gi, gc in w2v_batches(syn, world, W2V_SEED, n_steps=3):
        if pool is not None:
            model.set_pool(pool)
        model.step(gu[rank], gi[rank], gc[rank])
    p = model.saver.save(None, os.path.join(out_dir, 'ckpt'), global_step=model.steps)
    ni = (N_ITEMS - rank + world - 1) // world
    assert np.load(p + '.itemembed_cat_0.r%dof%d.npy' % (rank, world)).shape == (ni, D)       # no padding row
    assert np.load(p + '.itemembed_cat_0.Adagrad.r%dof%d.npy' % (rank, world)).shape == (ni, D)
    got = model.gather_global_tables(slots=True)
    if rank == 0:
        np.savez(os.path.join(out_dir, 'saved.npz'), **got)
    dist.barrier()
    with open(os.path.join(out_dir, "saved%d" % rank), "w") as f:
        f.write("ok")
    dist.destroy_process_group()


def _restore_worker(rank, world, port, out_dir, src_world):
    """A fresh model (another seed, its own random tables) at `world` restores what `src_world` ranks saved after
    three steps -- bit for bit -- and goes on for one step, against the oracle that ran the same four steps."""
    dist = _init(rank, world, port)
    from arx.utils.checkpoint import latest_checkpoint, read_manifest
    syn, params, tables = w2v_world()
    model = _model(rank, world, None, True, 'mw', seed=77)
    set_positives(model, syn, rank, world)
    path = latest_checkpoint(out_dir)
    assert read_manifest(path)['world'] == src_world
    ptrs = [t.data_ptr() for _, t, _, _ in model._checkpoint_arrays()]
    model.saver.restore(None, path)
    assert ptrs == [t.data_ptr() for _, t, _, _ in model._checkpoint_arrays()] and model.steps == 3
    saved = np.load(os.path.join(out_dir, 'saved.npz'))
    got = model.gather_global_tables(slots=True)
    assert set(got) == set(saved.files)
    for k in saved.files:
        assert _bitwise_equal(got[k], saved[k]), k
    ni = model.ni_loc
    assert not model.E_ctx[ni].any() and bool((model.A_ctx[ni] == float(np.float32(model.acc0))).all())
    ref = w2v_ref(syn, params, True, 'mw', B_LOC * src_world)
    old = w2v_batches(syn, src_world, W2V_SEED, n_steps=3)
    for pool, gu, gi, gc in old:
        ref_step(ref, pool, gu, gi, gc, False)
    model.set_pool(old[2][0])                                    # input data: the caller's, not saved
    _, gu, gi, gc = w2v_batches(syn, world, W2V_SEED + 1, n_steps=2)[1]
    l_ref = ref_step(ref, None, gu, gi, gc, False)
    model.step(gu[rank], gi[rank], gc[rank])
    l_got = float(model.read_loss().item())
    assert abs(l_got - l_ref) <= 1e-5 * abs(l_ref), (l_got, l_ref)
    compare_tables(model.gather_global_tables(slots=True), ref)
    with open(os.path.join(out_dir, "restored%d" % rank), "w") as f:
        f.write("ok")
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_w2v_save_world2_restore_world3(tmp_path):
    import torch.multiprocessing as mp
    port = 29360 + (os.getpid() % 400)
    mp.spawn(_save_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert all(os.path.exists(tmp_path / ("saved%d" % r)) for r in range(2))
    mp.spawn(_restore_worker, args=(3, port + 1, str(tmp_path), 2), nprocs=3, join=True)
    assert all(os.path.exists(tmp_path / ("restored%d" % r)) for r in range(3))


# ---------------------------------------------------------------------------------------- refusals, the two exports
def test_constructor_and_route_refusals():
    """Refused before any buffer, backend or process group is touched (the route: before anything is sent)."""
    from arx.dist import ShardedW2V
    from numpy_backend_w2v import NumpyW2VBackend
    base = (N_USERS, N_ITEMS, D, B_LOC, S)
    tail = (LR, 0, 1, 'cpu')
    for kind in ('bpr', 'bpr-hinge', 'warp'):
        with pytest.raises(ValueError, match="loss"):
            ShardedW2V(*base, N_IN, *tail, backend=object(), loss=kind)
    with pytest.raises(ValueError, match="exchange"):
        ShardedW2V(*base, N_IN, *tail, backend=object(), exchange='logits')
    for n in (0, -1):
        with pytest.raises(ValueError, match="n_input"):
            ShardedW2V(*base, n, *tail, backend=object())
    with pytest.raises(ValueError, match="tables"):
        ShardedW2V(*base, N_IN, *tail, backend=object(), tables={'user': np.zeros((N_USERS, D), np.float32)})
    _, _, tables = w2v_world()
    model = ShardedW2V(*base, N_IN, *tail, backend=NumpyW2VBackend(), tables=tables)     # (no process group exists)
    u, it = np.zeros(B_LOC, np.int32), np.arange(B_LOC, dtype=np.int32)
    ctx = np.zeros((N_IN, B_LOC), np.int32)
    bad = ctx.copy()
    bad[1, 2] = N_ITEMS
    neg = ctx.copy()
    neg[0, 0] = -1
    for args in ((u, it, bad), (u, it, neg), (u, it + N_ITEMS, ctx), (u, it - 1, ctx), (u, it, ctx[:2]),
                 (u, it, ctx[:, :4]), (u[:4], it[:4], ctx)):
        with pytest.raises(ValueError):
            model.prepare_route(*args)


def test_window_slots_kernels_validate_arguments_without_gpu():
    from arx import _lib
    lib = _lib.lib
    EINVAL, EUNSUPPORTED = -1, -4

    def err():
        m = lib.arx_last_error()
        return m.decode() if m else ""
    P = 4096          # (pointers are only compared with NULL and checked for alignment before the first HIP call)

    def fwd(R=P, ldr=68, slots=P, n=3, mb=8, d=64, base=P, ldb=64, out=P, ldo=64):
        return lib.arx_window_slots_fwd(R, ldr, slots, n, mb, d, 0.5, base, ldb, 0.5, out, ldo, None)

    def bwd(dX=P, ldx=64, slots=P, n=3, mb=8, d=64, dbase=P, ldbase=68, acc=0, dR=P, ldr=68):
        return lib.arx_window_slots_bwd(dX, ldx, slots, n, mb, d, 0.5, 0.5, dbase, ldbase, acc, dR, ldr, None)
    for bad in (dict(R=None), dict(slots=None), dict(out=None), dict(n=0), dict(mb=-1), dict(n=2, mb=1 << 30),
                dict(ldr=60), dict(ldr=66), dict(ldo=60), dict(ldo=66), dict(ldb=60), dict(ldb=66), dict(R=P + 4),
                dict(out=P + 8), dict(base=P + 4)):
        assert fwd(**bad) == EINVAL and "arx_window_slots_fwd" in err(), bad
    for bad in (dict(dX=None), dict(slots=None), dict(dbase=None), dict(dR=None), dict(n=0), dict(mb=-1),
                dict(n=2, mb=1 << 30), dict(ldx=60), dict(ldx=66), dict(ldbase=60), dict(ldbase=70), dict(ldr=60),
                dict(ldr=66), dict(dX=P + 4), dict(dbase=P + 8), dict(dR=P + 4), dict(acc=2)):
        assert bwd(**bad) == EINVAL and "arx_window_slots_bwd" in err(), bad
    for call, name in ((fwd, "arx_window_slots_fwd"), (bwd, "arx_window_slots_bwd")):
        for d in (62, 0, 260):
            assert call(d=d) == EUNSUPPORTED and name in err() and ("d=%d" % d) in err()
        assert call(mb=0) == 0
