"""What a forward tells its backward (rasterizer.ForwardNotes): the flags, and who may skip the backward's fills -- once, and
for a cached view only while no hit came in between.  CPU-only: no library, nothing is rasterized."""
import torch

from seganygaussians_amd import rasterizer as R


def test_claim_hands_the_prezeroed_buffers_out_once():
    pre = torch.zeros(4, 32)
    notes = R.ForwardNotes(8, prezero=pre, pack_zeroed=True)
    got, pack_zeroed = notes.claim()
    assert got is pre and pack_zeroed is True
    assert notes.claim() == (None, False)       # a second backward through a retained graph fills for itself
    assert notes.flags == 8


def test_a_hit_after_the_forward_takes_the_scratch_but_not_the_tensor():
    cell, pre = [0], torch.zeros(4, 32)
    notes = R.ForwardNotes(0, prezero=pre, pack_zeroed=True, epoch=cell)
    cell[0] += 1                                # a hit of this cached view came in
    got, pack_zeroed = notes.claim()
    assert got is pre and pack_zeroed is False
    untouched = R.ForwardNotes(0, prezero=pre, pack_zeroed=True, epoch=[0])   # no hit in between: both are the backward's
    got, pack_zeroed = untouched.claim()
    assert got is pre and pack_zeroed is True


def test_notes_of_a_cache_hit_never_report_pack_zeroed():
    pre = torch.zeros(4, 32)
    for notes in (R.ForwardNotes.for_hit(0), R.ForwardNotes.for_hit(16, pre)):
        assert notes.pack_zeroed is False
        assert notes.claim()[1] is False
    notes = R.ForwardNotes.for_hit(16, pre)
    assert notes.claim()[0] is pre and notes.claim() == (None, False)


def test_flags_of_reads_the_notes():
    buf = torch.empty(8, dtype=torch.uint8)
    assert R._flags_of(buf, None) == 0          # a bare tensor
    buf.mi_notes = R.ForwardNotes(128 | 8)
    assert R._flags_of(buf, None) == 136
    assert R._flags_of(buf, 1) == 1 and R._flags_of(buf, 0) == 0   # an explicit flags= wins
