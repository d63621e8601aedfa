"""The hand-built snappy frames of tests/snappy_frames.py against the oracle's restatement of the
reference Reader: every accepted frame decodes to its page, every rejected one raises. The same
lists go through the device decoder in tests/test_gpu_snappy.py."""
import pytest

from oracle import oracle as O
from tests import snappy_frames as F


@pytest.mark.parametrize("k", range(len(F.ACCEPTED)), ids=[c.name for c in F.ACCEPTED])
def test_accepted(k):
    payload, page = F.ACCEPTED[k].build(F.frame_id(k))
    assert O.snappy_framed_decode(payload) == page


@pytest.mark.parametrize("k", range(len(F.REJECTED)), ids=[c.name for c in F.REJECTED])
def test_rejected(k):
    payload, _ = F.REJECTED[k].build(F.frame_id(k))
    with pytest.raises(ValueError):
        O.snappy_framed_decode(payload)


def test_intact_twin_of_the_rejected_frames():
    payload, page = F.INTACT.build(F.frame_id(0))
    assert O.snappy_framed_decode(payload) == page


def test_frames_hold_what_they_are_named_for():
    """The tag bytes the lists promise are in the streams (a builder that quietly chose another
    spelling would test nothing)."""
    built = {c.name: c.build(F.frame_id(k))[0] for k, c in enumerate(F.ACCEPTED)}
    lit = built["literals"]
    assert bytes([59 << 2]) in lit and bytes([60 << 2, 60]) in lit and bytes([61 << 2, 0, 1]) in lit
    assert bytes([63 << 2, 1, 0, 0, 0]) in lit
    assert bytes([62 << 2, 0xFF, 0xFF, 0x00]) in built["full-block-three-byte-literal"]
    cp = built["copies"]
    assert F.copy_bytes(1, 1, 11) in cp and F.copy_bytes(1, 2047, 8) == bytes([0xF1, 0xFF]) and bytes([0xF1, 0xFF]) in cp
    assert F.copy_bytes(2, 2100, 64) in cp and F.copy_bytes(4, 300, 40) in cp
    assert built["varint-padded-to-6"][18:24] == bytes([0xED, 0x88, 0x80, 0x80, 0x80, 0x00])
    assert len(F.ACCEPTED[3].build(F.frame_id(3))[1]) == 65_537
