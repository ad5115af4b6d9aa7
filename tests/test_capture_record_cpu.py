"""ops.CapturedGraph.record / replay and ops.joined are the one implementation of step-graph capture, feed swap and
stream join.  Checked without a GPU, as test_capture_gc_cpu.py does: the C entry points are replaced by a recorder
(the fake arx_capture_end_feeds / arx_graph_feed_dst0 fill their out-parameters through the byref objects)."""
import gc

import pytest
import torch


def _feeds(n):
    """n (src, dst) pairs of 4-byte host tensors: only their addresses and sizes travel."""
    return [(torch.zeros(4 + k, dtype=torch.int32), torch.zeros(4 + k, dtype=torch.int32)) for k in range(n)]


@pytest.fixture
def recorder(monkeypatch):
    from arx import ops
    seen = []           # (name, gc enabled) per C call
    detail = []         # (name, what the call carried)
    state = {"dst0": [], "fail_end": False}

    def fake_call(name, *args):
        seen.append((name, gc.isenabled()))
        if name == "arx_copy_words":
            detail.append((name, [int(args[2][a]) for a in range(args[0])]))
        elif name in ("arx_capture_end", "arx_capture_end_feeds"):
            if state["fail_end"]:
                raise RuntimeError("end failed")
            if name == "arx_capture_end_feeds":
                args[3]._obj.value = len(state["dst0"])
        elif name == "arx_graph_feed_dst0":
            args[2]._obj.value = state["dst0"][args[1]]
        elif name == "arx_graph_set_feed":
            idx, n = args[2], args[3]
            detail.append((name, idx, n, [int(args[4][a]) for a in range(n)]))
        return 0
    monkeypatch.setattr(ops, "call", fake_call)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    return ops, seen, detail, state


def _names(seen):
    return [n for n, _ in seen]


def _recorded(ops, state, feeds, body=lambda: None):
    """record() over `feeds`; the fake graph reports one feed node per group of eight, last group first."""
    state["dst0"] = [feeds[k][1].data_ptr() for k in range(0, len(feeds), 8)][::-1]
    return ops.CapturedGraph.record(body, feeds)


def test_record_order_feed_groups_and_gc(recorder):
    ops, seen, detail, state = recorder
    feeds = _feeds(10)                                   # two groups: 8 + 2
    assert gc.isenabled()
    g = _recorded(ops, state, feeds, body=lambda: ops.call("body_kernel"))
    assert gc.isenabled()
    assert _names(seen) == ["arx_capture_begin", "arx_copy_words", "arx_copy_words", "body_kernel",
                            "arx_capture_end_feeds", "arx_graph_feed_dst0", "arx_graph_feed_dst0"]
    assert not any(on for _, on in seen)                 # no collection anywhere inside the capture
    assert [d[1] for d in detail] == [[d_.data_ptr() for _, d_ in feeds[:8]], [d_.data_ptr() for _, d_ in feeds[8:]]]
    assert g.feed_groups == [tuple((d_.data_ptr(), d_.numel()) for _, d_ in feeds[:8]),
                             tuple((d_.data_ptr(), d_.numel()) for _, d_ in feeds[8:])]
    assert g.feeds_match(feeds) and not g.feeds_match(feeds[:8])


def test_record_without_feeds_ends_plainly(recorder):
    ops, seen, _, _ = recorder
    g = ops.CapturedGraph.record(lambda: ops.call("body_kernel"))
    assert _names(seen) == ["arx_capture_begin", "body_kernel", "arx_capture_end"]
    assert g.feed_groups is None and gc.isenabled()


def test_record_body_error_outlives_a_failing_end(recorder):
    """The body's exception is the one that surfaces, although ending the (invalidated) capture raises as well."""
    ops, seen, _, state = recorder

    def body():
        state["fail_end"] = True
        raise KeyError("body")
    with pytest.raises(KeyError):
        ops.CapturedGraph.record(body, _feeds(2))
    assert _names(seen).count("arx_capture_end") + _names(seen).count("arx_capture_end_feeds") == 1
    assert gc.isenabled()


def test_record_end_error_propagates(recorder):
    ops, seen, _, state = recorder
    state["fail_end"] = True
    with pytest.raises(RuntimeError, match="end failed"):
        ops.CapturedGraph.record(lambda: None, _feeds(2))
    assert _names(seen)[-1] == "arx_capture_end_feeds" and gc.isenabled()
    state["fail_end"], state["dst0"] = False, []         # ... and so does a feed node that was not found
    with pytest.raises(RuntimeError, match="feed node"):
        ops.CapturedGraph.record(lambda: None, _feeds(2))
    assert gc.isenabled()


def test_replay_matching_feeds_swaps_sources(recorder):
    ops, seen, detail, state = recorder
    feeds = _feeds(10)
    g = _recorded(ops, state, feeds)
    del seen[:], detail[:]
    other = [(torch.zeros_like(d_), d_) for _, d_ in feeds]          # same destinations, fresh sources
    g.replay(other)
    assert _names(seen) == ["arx_graph_set_feed", "arx_graph_set_feed", "arx_graph_launch"]
    # group 0 lives in node 1, group 1 in node 0 (the fake graph lists its feed nodes last group first)
    assert detail == [("arx_graph_set_feed", 1, 8, [s_.data_ptr() for s_, _ in other[:8]]),
                      ("arx_graph_set_feed", 0, 2, [s_.data_ptr() for s_, _ in other[8:]])]


def test_replay_other_destinations_feeds_eagerly(recorder):
    ops, seen, detail, state = recorder
    g = _recorded(ops, state, _feeds(10))
    del seen[:], detail[:]
    other = _feeds(3)
    g.replay(other)
    assert _names(seen) == ["arx_copy_words", "arx_graph_set_feed", "arx_graph_set_feed", "arx_graph_launch"]
    assert detail == [("arx_copy_words", [d_.data_ptr() for _, d_ in other]),
                      ("arx_graph_set_feed", 1, 0, []), ("arx_graph_set_feed", 0, 0, [])]


def test_replay_none_clears_once_and_is_bare_without_feed_nodes(recorder):
    ops, seen, detail, state = recorder
    feeds = _feeds(2)
    g = _recorded(ops, state, feeds)
    g.replay(feeds)
    del seen[:], detail[:]
    g.replay(None)                                       # after a fed replay: the nodes must not re-copy
    assert _names(seen) == ["arx_graph_set_feed", "arx_graph_launch"]
    assert detail == [("arx_graph_set_feed", 0, 0, [])]
    del seen[:]
    g.replay([])                                         # nothing live any more: the launch alone
    assert _names(seen) == ["arx_graph_launch"]
    bare = ops.CapturedGraph.record(lambda: None)
    del seen[:]
    bare.replay(None)
    assert _names(seen) == ["arx_graph_launch"]


def test_joined_none_touches_no_stream(recorder, monkeypatch):
    ops, seen, _, _ = recorder

    def no_cuda(*a, **k):
        raise AssertionError("torch.cuda used by joined(None)")
    for name in ("current_stream", "stream", "Stream"):
        monkeypatch.setattr(torch.cuda, name, no_cuda)
    ran = []
    with ops.joined(None):
        ran.append(1)
    assert ran == [1] and seen == []
    with pytest.raises(KeyError):                        # the block's exception passes through
        with ops.joined(None):
            raise KeyError("x")
