"""CPU: the helpers of hierarchicalgnn_amd._lib that the loss operators share: the device-keyed accumulator of
unread status words (CPU int32 tensors stand in for the device words) and the workspace query."""
import pytest
import torch

from hierarchicalgnn_amd import _lib

D0, D1 = torch.device("cuda", 0), torch.device("cuda", 1)


def _word(v):
    return torch.tensor([v], dtype=torch.int32)


def test_pending_status_ors_per_device_and_pops_on_read():
    stats = {"host_reads": 0, "other": 7}
    pending = _lib.PendingStatus(stats)
    assert pending.take() == 0 and pending.take(D0) == 0 and stats["host_reads"] == 0      # nothing pending: no read
    pending.add(D0, _word(1))
    pending.add(D0, _word(4))
    pending.add(D0, _word(1))
    pending.add(D1, _word(2))
    assert pending.take(D0) == 5 and stats["host_reads"] == 1                              # D0's words, OR-ed; one read
    assert pending.take(D0) == 0 and stats["host_reads"] == 1                              # cleared, and not counted
    assert pending.take("cuda:1") == 2 and stats["host_reads"] == 2                        # D1's word was left alone
    pending.add(D0, _word(8))
    pending.add(D1, _word(2))
    pending.add(D1, _word(16))
    assert pending.take() == 26 and stats["host_reads"] == 4                               # every device, one read each
    assert pending.take() == 0 and stats["host_reads"] == 4
    assert stats["other"] == 7


def test_the_two_loss_modules_keep_separate_counters():
    from hierarchicalgnn_amd import edge_classifier, embedding
    assert embedding.stats is not edge_classifier.stats
    assert list(embedding.stats) == ["host_reads"] == list(edge_classifier.stats)
    assert embedding._ph_pending.stats is embedding.stats and edge_classifier._wb_pending.stats is edge_classifier.stats
    before = edge_classifier.stats["host_reads"]
    embedding._ph_pending.add(D0, _word(0))
    reads = embedding.stats["host_reads"]
    embedding.pair_hinge_check(D0)                                                         # word 0: clean, one read
    assert embedding.stats["host_reads"] == reads + 1 and edge_classifier.stats["host_reads"] == before
    embedding._ph_pending.add(D0, _word(1))
    with pytest.raises(ValueError, match="pair_hinge_loss: a pair id is negative"):
        embedding.pair_hinge_check()
    edge_classifier._wb_pending.add(D1, _word(_lib.WB_ST_BAD_SCORE))
    with pytest.raises(ValueError, match="weighted_bce_loss: a score is NaN"):
        edge_classifier.weighted_bce_check(D1)
    edge_classifier.weighted_bce_check()                                                   # cleared by the read above


def test_workspace_raises_the_library_message_when_the_size_query_fails():
    with pytest.raises(RuntimeError, match=r"hgnn_pair_hinge_workspace_bytes failed .*1 <= D <= 16"):
        _lib.workspace("hgnn_pair_hinge_workspace_bytes", "cpu", 10, 10, 0, 0)             # D = 0: host-side refusal

