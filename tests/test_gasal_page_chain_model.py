"""The page-chain model (tests/gasal_page_chain_model.py) on chains worked out by hand from the
reference's host_batch.cpp:79-153 (fill), :162-223 (add), :60-70 (reset) and gasal_align.cu:70-175.
States are (offset, data_size, page_size, locked) per page."""
import pytest

from gasal_page_chain_model import N_CODE, PageChain, grown, pad8


def _slot(data):
    return bytes(data) + bytes([N_CODE]) * (pad8(len(data)) - len(data))


def test_first_page_of_init_streams():
    # ctors.cpp:33-38: max_n_alns * pad8(max_len)
    assert PageChain.for_streams(16, 4).states() == [(0, 0, 64, 0)]
    assert PageChain.for_streams(24, 4).states() == [(0, 0, 96, 0)]
    assert PageChain.for_streams(17, 3).total_bytes == 72


def test_growth_64_128_256():
    c = PageChain(64)
    idx = 0
    for k in range(7):                       # 7 slots of 8: 56 of 64
        idx = c.fill(idx, bytes([65 + k]) * 5)
    assert idx == 56 and c.states() == [(0, 56, 64, 0)] and c.total_bytes == 64
    idx = c.fill(idx, b"C" * 12)             # 16 > 8 left: page 2 of 128 at 56, page 1 locked
    assert idx == 72 and c.states() == [(0, 56, 64, 1), (56, 16, 128, 0)] and c.total_bytes == 192
    for _ in range(2):                       # 16 + 2 * 40 = 96 of 128
        idx = c.fill(idx, b"G" * 40)
    assert idx == 152 and c.states()[1] == (56, 96, 128, 0)
    idx = c.fill(idx, b"T" * 33)             # 40 > 32 left: page 3 of 256 at 56 + 96
    assert idx == 192
    assert c.states() == [(0, 56, 64, 1), (56, 96, 128, 1), (152, 40, 256, 0)] and c.total_bytes == 448
    # the 8 bytes left on page 1 and the 32 left on page 2 are in no page's data_size: idx has no holes
    img = c.image()
    assert len(img) == 192
    assert img[56:72] == _slot(b"C" * 12) and img[152:192] == _slot(b"T" * 33)
    assert img[:8] == _slot(b"A" * 5) and img[48:56] == _slot(b"G" * 5)


def test_exact_fill_opens_no_page():
    c = PageChain(64)
    idx = c.fill(0, b"A" * 24)
    idx = c.fill(idx, b"C" * 40)             # 24 + 40 = 64: exactly the page
    assert idx == 64 and c.states() == [(0, 64, 64, 0)] and c.total_bytes == 64
    idx = c.fill(idx, b"G")                  # the next slot opens page 2 at 64
    assert idx == 72 and c.states() == [(0, 64, 64, 1), (64, 8, 128, 0)]
    assert c.image() == _slot(b"A" * 24) + b"C" * 40 + _slot(b"G")


def test_one_byte_over():
    # 57 bases need a 64-byte slot and fit the page; 65 need 72 and do not
    c = PageChain(64)
    assert c.fill(0, b"A" * 57) == 64 and c.states() == [(0, 64, 64, 0)]
    c = PageChain(64)
    assert c.fill(0, b"A" * 65) == 72
    assert c.states() == [(0, 0, 64, 1), (0, 72, 128, 0)]      # page 1 locked and empty, page 2 at 0
    # a slot one byte over what is left: 56 used, 9 bases need 16
    c = PageChain(64)
    idx = c.fill(0, b"A" * 56)
    assert c.fill(idx, b"C" * 8) == 64 and c.states() == [(0, 64, 64, 0)]
    c = PageChain(64)
    idx = c.fill(0, b"A" * 56)
    assert c.fill(idx, b"C" * 9) == 72 and c.states() == [(0, 56, 64, 1), (56, 16, 128, 0)]


def test_reuse_after_reset():
    c = PageChain(64)
    idx = 0
    for n in (30, 30, 100, 30, 200):         # slots 32 32 | 104 | (32 > 24 left) 32 200
        idx = c.fill(idx, b"A" * n)
    assert c.states() == [(0, 64, 64, 1), (64, 104, 128, 1), (168, 232, 256, 0)] and idx == 400
    c.reset()
    assert c.states() == [(0, 0, 64, 0), (0, 0, 128, 0), (0, 0, 256, 0)] and c.total_bytes == 448
    assert c.image() == b""
    # a round that fits page 1 leaves the later pages at data_size 0: nothing of them is uploaded
    idx = c.fill(0, b"C" * 20)
    idx = c.fill(idx, b"G" * 40)
    assert idx == 64 and c.states() == [(0, 64, 64, 0), (0, 0, 128, 0), (0, 0, 256, 0)]
    assert c.image() == _slot(b"C" * 20) + b"G" * 40
    c.reset()
    # a large round walks the existing pages (:127-134): offsets are rewritten, no page is added
    idx = c.fill(0, b"T" * 40)               # page 1: 40 of 64
    idx = c.fill(idx, b"A" * 30)             # 32 > 24 left: page 2 at 40
    assert c.states() == [(0, 40, 64, 1), (40, 32, 128, 0), (0, 0, 256, 0)]
    idx = c.fill(idx, b"C" * 96)             # exactly the rest of page 2
    assert c.states()[1] == (40, 128, 128, 0)
    idx = c.fill(idx, b"G" * 8)              # page 3 at 40 + 128
    assert idx == 176 and c.states() == [(0, 40, 64, 1), (40, 128, 128, 1), (168, 8, 256, 0)]
    assert c.total_bytes == 448 and len(c.pages) == 3
    assert c.image() == b"T" * 40 + _slot(b"A" * 30) + b"C" * 96 + b"G" * 8


def test_oversized_sequence_is_dropped_silently():
    # pinned reference behaviour (host_batch.cpp:137): no else branch
    c = PageChain(64)
    idx = c.fill(0, b"A" * 16)
    assert c.fill(idx, b"C" * 200) == idx                       # 200 > 128: nothing written, idx unchanged
    assert c.states() == [(0, 16, 64, 1), (16, 0, 128, 0)] and c.total_bytes == 192
    assert c.image() == b"A" * 16
    # the same sequence again: page 2 is the last page now, page 3 of 256 takes it
    assert c.fill(idx, b"C" * 200) == idx + 200
    assert c.states() == [(0, 16, 64, 1), (16, 0, 128, 1), (16, 200, 256, 0)]
    # on a reused chain the walk makes one step per call: the successor is too small, nothing is written
    c.reset()
    assert c.fill(0, b"G" * 200) == 0
    assert c.states() == [(0, 0, 64, 1), (0, 0, 128, 0), (0, 0, 256, 0)]
    assert c.fill(0, b"G" * 200) == 200
    assert c.states() == [(0, 0, 64, 1), (0, 0, 128, 1), (0, 200, 256, 0)]


def test_add_is_not_counted_in_data_size():
    # pinned reference behaviour (host_batch.cpp:188-194): add() writes bytes and nothing else
    c = PageChain(64)
    idx = 0
    for k in range(6):
        idx = c.add(idx, bytes([65 + k]) * 10)
    assert idx == 60 and c.states() == [(0, 0, 64, 0)] and c.total_bytes == 64
    assert bytes(c.pages[0].data[:60]) == b"".join(bytes([65 + k]) * 10 for k in range(6))
    assert c.image() == b""                                     # nothing would be uploaded
    idx = c.add(idx, b"T" * 10)                                 # 70 > 64: page of 128 at 60, nothing locked
    assert idx == 70 and c.states() == [(0, 0, 64, 0), (60, 0, 128, 0)] and c.total_bytes == 128
    assert bytes(c.pages[1].data[:10]) == b"T" * 10 and c.getlast() == 1
    idx = c.add(idx, b"g")                                      # addbase: walks to page 2 (its offset 60 < 71)
    assert idx == 71 and c.pages[1].data[10] == ord("g")
    assert c.add(5, b"xy") == 7 and bytes(c.pages[0].data[5:7]) == b"xy"   # below page 2's offset: page 1
    # past the total: the new page replaces page 2 behind the first page (:216)
    idx = c.add(120, b"N" * 10)
    assert idx == 130 and c.states() == [(0, 0, 64, 0), (120, 0, 256, 0)] and c.total_bytes == 256
    assert c.getlast() == 1


def test_add_first_allocation_smaller_than_a_sequence():
    c = PageChain(8)                                            # :211-212: doubles until one sequence fits
    assert c.add(0, b"A" * 50) == 50
    assert c.states() == [(0, 0, 8, 0), (0, 0, 64, 0)] and c.total_bytes == 64


def test_page_write_bounds_are_checked():
    c = PageChain(64)
    with pytest.raises(IndexError):
        c.pages[0]._write(60, b"12345")


def test_device_growth_factor():
    # gasal_align.cu:72-77: the smallest i >= 2 with cap * i >= need
    assert grown(64, 64) == 64 and grown(64, 8) == 64
    assert grown(64, 72) == 128 and grown(64, 128) == 128       # factor 2 up to exactly 2 * cap
    assert grown(64, 136) == 192 and grown(64, 392) == 448      # 8 bytes more: factor 3
    assert grown(4, 8) == 8 and grown(4, 9) == 12 and grown(4, 14) == 16
