"""The full-vocabulary serving rules of arx.topk, without a device: when the logits are streamed, which top-k node
recommends, and the chunked re-run after an overflow.  Expected values are literals worked out from the expression
the models carried before the rules had one owner:
    k <= 1024 and (rows * V * 4 > ARX_STREAM_TOPK_BYTES (default 1 << 30) or (V > 65536 and d in (32, 64, 128)))
for logits that are a plain Prediction, never otherwise.
"""
import types

import pytest
import torch


@pytest.mark.parametrize("args, expect", [
    ((64, 1_000_000, 100, 128, True), True),        # 256 MB, under 1 GB, but the fused form applies
    ((64, 60_000, 100, 128, True), False),
    ((1024, 1_000_000, 100, 48, True), True),       # 4.1 GB
    ((64, 1_000_000, 100, 48, True), False),
    ((64, 1_000_000, 2000, 128, True), False),      # k > 1024
    ((1024, 1_000_000, 100, 128, False), False),    # not a plain prediction
])
def test_streams_topk_default_threshold(monkeypatch, args, expect):
    from arx import topk
    monkeypatch.delenv('ARX_STREAM_TOPK_BYTES', raising=False)
    assert topk.stream_min_bytes() == 1 << 30
    assert topk.streams_topk(*args) is expect


def test_threshold_is_read_at_call_time(monkeypatch):
    from arx import topk                             # imported BEFORE the variable is set
    monkeypatch.delenv('ARX_STREAM_TOPK_BYTES', raising=False)
    assert topk.streams_topk(32, 4800, 30, 32, True) is False
    assert topk.logits_too_big(16, 500) is False
    monkeypatch.setenv('ARX_STREAM_TOPK_BYTES', '0')
    assert topk.streams_topk(32, 4800, 30, 32, True) is True
    monkeypatch.setenv('ARX_STREAM_TOPK_BYTES', '1')
    assert topk.logits_too_big(16, 500) is True
    assert topk.logits_too_big(0, 500) is False      # 0 bytes are not more than 1


def _scan(overflow):
    """A TopKScan without its device buffers: fused, overflowed() and chunked() are the class's own."""
    from arx.topk import TopKScan

    class Scan(TopKScan):
        def __init__(self):
            self.fused = True
            self.overflow = torch.full((1,), overflow, dtype=torch.int32)
    return Scan()


class _Calls(object):
    def __init__(self, scan, fail_on=None):
        self.scan, self.fail_on = scan, fail_on
        self.runs, self.forgets = [], 0

    def run(self):
        self.runs.append(self.scan.fused)            # the setting this run saw
        if len(self.runs) == self.fail_on:
            raise RuntimeError("run %d" % self.fail_on)
        return len(self.runs)

    def forget(self):
        self.forgets += 1


def test_run_complete_without_overflow_runs_once():
    from arx.topk import run_complete
    scan = _scan(0)
    c = _Calls(scan)
    assert run_complete(scan, c.run, c.forget) == 1
    assert c.runs == [True] and c.forgets == 0 and scan.fused is True


def test_run_complete_after_overflow_runs_again_chunked():
    from arx.topk import run_complete
    scan = _scan(3)
    c = _Calls(scan)
    assert run_complete(scan, c.run, c.forget) == 2
    assert c.runs == [True, False]                   # fused, then chunked
    assert c.forgets == 2 and scan.fused is True
    c2 = _Calls(scan)
    run_complete(scan, c2.run)                       # forget is optional
    assert c2.runs == [True, False] and scan.fused is True


def test_run_complete_restores_when_the_second_run_raises():
    from arx.topk import run_complete
    scan = _scan(1)
    c = _Calls(scan, fail_on=2)
    with pytest.raises(RuntimeError, match="run 2"):
        run_complete(scan, c.run, c.forget)
    assert c.runs == [True, False] and c.forgets == 2 and scan.fused is True


def test_run_complete_dense_node_runs_once():
    from arx.topk import run_complete
    c = _Calls(types.SimpleNamespace(fused=None))    # no overflowed(): a dense TopK / TopKSoftmax
    assert run_complete(c.scan, c.run, c.forget) == 1
    assert c.runs == [None] and c.forgets == 0


def test_chunked_restores_the_setting_it_found():
    scan = _scan(0)
    scan.fused = False                               # (ARX_TOPK_FUSED=0, or a width the fused kernel does not take)
    with scan.chunked():
        assert scan.fused is False
    assert scan.fused is False


def test_eval_masks_of_a_sampled_model():
    from arx import graph as G
    from arx.attributes.embed_attribute import EVAL_LOSS_OF, EmbeddingAttribute
    assert EVAL_LOSS_OF == {'mw': 'warp', 'mce': 'ce'}
    m = types.SimpleNamespace(mask={'mw': 'MW', 'warp': 'WARP'})
    dense, streamed = object(), object.__new__(G.StreamEvalLoss)
    masks = lambda loss, node: EmbeddingAttribute.eval_masks(m, loss, node)
    assert masks('mw', dense) == ['WARP']
    assert masks('mw', streamed) == []               # the streamed loss reads the positives CSR itself
    assert masks('mce', dense) == []                 # 'ce' has no mask
    assert masks('warp', dense) == ['WARP']
    assert masks('ce', dense) == []
