"""Plain-Python model of GASAL2's extensible host batch: the chain of pinned pages that
gasal_host_batch_fill / gasal_host_batch_add write and gasal_aln_async uploads (TEST
INFRASTRUCTURE ONLY).

Written from the reference host code, not from genomics-gpu_amd/csrc/gasal_api.cpp:
  Non-CDP/GASAL2/src/host_batch.cpp:11-22    gasal_host_batch_new: a page of page_size bytes at `offset`
  Non-CDP/GASAL2/src/host_batch.cpp:60-70    reset: data_size = offset = is_locked = 0 on every page
  Non-CDP/GASAL2/src/host_batch.cpp:79-153   fill
  Non-CDP/GASAL2/src/host_batch.cpp:162-223  add (addbase, :156-159, is add of one byte)
  Non-CDP/GASAL2/src/gasal_align.cu:152-175  upload: data_size bytes of every page to device
                                             position `offset`, page after page
  Non-CDP/GASAL2/src/gasal_align.cu:70-145   device growth: the smallest factor i >= 2 with cap * i >= need
  Non-CDP/GASAL2/src/ctors.cpp:33-38         first page: max_n_alns * pad8(max_len) bytes

fill(idx, data), restated (:100-152).  need = len(data) rounded up to 8; the pad bytes are N_CODE.
  1. skip the locked pages (:104-105);
  2. on the last page, when need does not fit what is left of it: append a page of twice its size
     at offset = this page's offset + data_size, lock this page, add the new size to the total,
     step onto the new page (:107-125);
  3. on a page that has a successor, when need does not fit: set the successor's offset to this
     page's offset + data_size, lock this page, step onto the successor (:127-134).  Only one
     step: a reused chain is walked one page per call;
  4. when need fits the page now current: write at idx - offset, data_size += need, idx += need
     (:137-150).
Two rules of the reference that look odd are kept as they are, since callers see them:
  * step 4 has no else.  A sequence that does not fit even the doubled page (or, on a reused
    chain, the successor) writes nothing and returns idx unchanged; the page opened for it stays
    in the chain, empty, and the pages before it stay locked (:137).  Nothing is reported.
  * add() never touches data_size (:188-194).  gasal_aln_async uploads data_size bytes per
    page, so bytes written through add / addbase alone are not uploaded, and image() leaves
    them out.  add() also never locks a page and places its new page at `idx` with the whole
    doubled total as its size (:208-214).
One more consequence of add()'s loop is modelled as it is written: the walk only moves on while the
total covers idx + size, so an add past the total grows the chain from the page the walk stands
on, which is the first page; `cur_page->next = res` (:216) then replaces whatever followed that page.
A chain grown by add() alone therefore never has more than two pages.
"""
from __future__ import annotations

N_CODE = 0x4E


def pad8(n: int) -> int:
    return (n + 7) // 8 * 8


class Page:
    def __init__(self, page_size: int, offset: int):
        self.page_size = page_size
        self.offset = offset
        self.data_size = 0
        self.locked = 0
        self.data = bytearray(page_size)
        self.written = bytearray(page_size)     # 1 where a byte was written (pinned memory starts undefined)

    def state(self):
        return (self.offset, self.data_size, self.page_size, self.locked)

    def _write(self, at: int, data: bytes):
        if at < 0 or at + len(data) > self.page_size:
            raise IndexError(f"write of {len(data)} bytes at {at} leaves a page of {self.page_size}")
        self.data[at:at + len(data)] = data
        self.written[at:at + len(data)] = b"\x01" * len(data)


class PageChain:
    """One side (query or target) of a storage.  total_bytes is host_max_{query,target}_batch_bytes."""

    def __init__(self, first_page_bytes: int):
        self.pages = [Page(first_page_bytes, 0)]
        self.total_bytes = first_page_bytes

    @classmethod
    def for_streams(cls, max_len: int, max_n_alns: int):
        """The first page gasal_init_streams makes (ctors.cpp:33-38)."""
        return cls(max_n_alns * pad8(max_len))

    def states(self):
        return [p.state() for p in self.pages]

    def reset(self):
        for p in self.pages:
            p.data_size = 0; p.offset = 0; p.locked = 0

    def fill(self, idx: int, data: bytes) -> int:
        size = len(data)
        need = pad8(size)
        k = 0
        while self.pages[k].locked:                                             # :104-105
            k += 1
        cur = self.pages[k]
        if k == len(self.pages) - 1 and cur.page_size - cur.data_size < need:   # :107-125
            self.pages.append(Page(cur.page_size * 2, cur.offset + cur.data_size))
            cur.locked = 1
            self.total_bytes += cur.page_size * 2
            k += 1
            cur = self.pages[k]
        if k < len(self.pages) - 1 and cur.page_size - cur.data_size < need:    # :127-134
            self.pages[k + 1].offset = cur.offset + cur.data_size
            cur.locked = 1
            k += 1
            cur = self.pages[k]
        if cur.page_size - cur.data_size >= need:                               # :137-150
            cur._write(idx - cur.offset, bytes(data) + bytes([N_CODE]) * (need - size))
            idx += need
            cur.data_size += need
        return idx

    def add(self, idx: int, data: bytes) -> int:
        size = len(data)
        k = 0
        while True:                                                             # :186-220
            cur = self.pages[k]
            nxt = self.pages[k + 1] if k + 1 < len(self.pages) else None
            if self.total_bytes >= idx + size and (nxt is None or nxt.offset >= idx + size):
                cur._write(idx - cur.offset, bytes(data))
                return idx + size
            if self.total_bytes >= idx + size and nxt is not None and nxt.offset < idx + size:
                k += 1
                continue
            self.total_bytes += self.total_bytes                                # :208
            while self.total_bytes < size:                                      # :211-212
                self.total_bytes += self.total_bytes
            # :214-218: linked behind the page the walk stands on, whatever followed it before
            self.pages = self.pages[:k + 1] + [Page(self.total_bytes, idx)]
            k += 1

    def getlast(self) -> int:
        return len(self.pages) - 1

    def image(self) -> bytes:
        """What the per-page copies of gasal_aln_async assemble on the device: data_size bytes of
        each page at its offset, in chain order (a later page overwrites an earlier one)."""
        end = max((p.offset + p.data_size for p in self.pages), default=0)
        img = bytearray(end)
        for p in self.pages:
            img[p.offset:p.offset + p.data_size] = p.data[:p.data_size]
        return bytes(img)


def grown(cap: int, need: int) -> int:
    """gpu_max_* after gasal_aln_async saw `need` (gasal_align.cu:70-77, :93-100, :111-118)."""
    if cap >= need:
        return cap
    i = 2
    while cap * i < need:
        i += 1
    return cap * i
