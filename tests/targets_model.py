"""`openge targets` in plain Python: the definition of DESIGN.md section 25, the yardstick of csrc/targets.hip.

Realignment target intervals from the reads' own indels (RealignerTargetCreator at its defaults, without
mismatch-entropy events and known indels).  Coordinates are 1-based and closed.

  reads used  FLAG has none of 0x4, 0x100, 0x200, 0x400; MAPQ neither 0 nor 255; refID >= 0 and pos >= 0; not a bad
              mate (FLAG 0x1 set, 0x8 clear, mate refID != refID).  Such a read with refID >= n_ref, a CIGAR that
              does not fit its block_size or an op code above 8 is an error that names the record (the lowest one;
              of one record the first of the three).
  events      first / last = the read's first and last M, = or X op; every I or D op strictly between them is an
              event at a = pos + (lengths of the M, D, N, =, X ops before it): an insertion (refID, a, a + 1), a
              deletion of L (refID, a, a + L); the stop is clipped to the contig's length (a length below 0 counts
              as 0); a start beyond 2^31 - 1 is stored as 2^31 - 1.
  merge       events sorted by (refID, start, stop); an event joins the current interval when it has its refID and
              start <= interval stop + gap, the stop becomes the larger one; n_events = the events that joined.
  drop        an interval with stop - start >= max_interval is dropped.
  output      the kept intervals in (refID, start) order as (refID, start, stop, n_events) and as lines
              "contig:start-stop\\n".
"""
from __future__ import annotations

import struct
from dataclasses import dataclass

import numpy as np

ALIGNED = (0, 7, 8)          # M = X
CONSUMES_REF = (0, 2, 3, 7, 8)  # M D N = X
SKIP_FLAGS = 0x4 | 0x100 | 0x200 | 0x400
EVENT_LIMIT = 2**32 - 1
I32_MAX = 2**31 - 1


class TargetsError(ValueError):
    """OGE_ERR_ARG of the model; .record is the record the message names, .kind 0 refID, 1 CIGAR size, 2 op code"""

    def __init__(self, record: int, kind: int):
        self.record, self.kind = record, kind
        super().__init__(f"targets: record {record} {BAD[kind]}")


class TargetsLimit(ValueError):
    pass


BAD = ("passes the read filter with a refID outside [0, n_ref)", "has a CIGAR that does not fit its block_size",
       "has a CIGAR op code above 8")


@dataclass
class Result:
    reads_used: int
    events: int
    intervals: int
    dropped_long: int
    targets: int
    text_bytes: int
    array: np.ndarray   # (targets, 4) int64: refID, start, stop, n_events
    text: bytes

    def counters(self) -> dict:
        return {k: getattr(self, k) for k in ("reads_used", "events", "intervals", "dropped_long", "targets", "text_bytes")}


def read_events(rb: bytes, index: int, ref_lens) -> list[tuple[int, int, int]] | None:
    """The events of one record (block_size field included); None when the read is not used."""
    bs, refid, pos, lname, mapq, _bin, ncig, flag, _lseq, mref = struct.unpack_from("<IiiBBHHHii", rb, 0)
    if flag & SKIP_FLAGS or mapq in (0, 255) or refid < 0 or pos < 0:
        return None
    if flag & 0x1 and not flag & 0x8 and mref != refid:
        return None
    if refid >= len(ref_lens):
        raise TargetsError(index, 0)
    if 36 + lname + 4 * ncig > 4 + bs:
        raise TargetsError(index, 1)
    ops = struct.unpack_from(f"<{ncig}I", rb, 36 + lname)
    if any(op & 0xF > 8 for op in ops):
        raise TargetsError(index, 2)
    aligned = [j for j, op in enumerate(ops) if op & 0xF in ALIGNED]
    out: list[tuple[int, int, int]] = []
    if not aligned:
        return out
    first, last = aligned[0], aligned[-1]
    clip = max(int(ref_lens[refid]), 0)
    consumed = 0
    for j, op in enumerate(ops):
        code, ln = op & 0xF, op >> 4
        if first < j < last and code in (1, 2):
            a = pos + consumed
            stop = a + 1 if code == 1 else a + ln
            out.append((refid, min(a, I32_MAX), min(stop, clip)))
        if code in CONSUMES_REF:
            consumed += ln
    return out


def merge(events, gap: int = 0) -> list[list[int]]:
    """[(refID, start, stop)] in any order -> [[refID, start, stop, n_events]]"""
    out: list[list[int]] = []
    for rid, start, stop in sorted(events):
        if out and out[-1][0] == rid and start <= out[-1][2] + gap:
            out[-1][2] = max(out[-1][2], stop)
            out[-1][3] += 1
        else:
            out.append([rid, start, stop, 1])
    return out


def targets(records: list[bytes], refs, max_interval: int = 500, gap: int = 0) -> Result:
    """records: BAM records as bytes; refs: [(name, length)]"""
    if max_interval < 1 or gap < 0:
        raise ValueError("targets: max_interval < 1 or gap < 0")
    lens = [ln for _, ln in refs]
    events, used = [], 0
    for i, rb in enumerate(records):
        ev = read_events(rb, i, lens)
        if ev is None:
            continue
        used += 1
        events += ev
    if len(events) >= EVENT_LIMIT:
        raise TargetsLimit("targets: 2^32-1 or more events")
    ivs = merge(events, gap)
    kept = [iv for iv in ivs if iv[2] - iv[1] < max_interval]
    text = "".join(f"{refs[r][0]}:{a}-{b}\n" for r, a, b, _ in kept).encode()
    return Result(used, len(events), len(ivs), len(ivs) - len(kept), len(kept), len(text),
                  np.array(kept, dtype=np.int64).reshape(len(kept), 4), text)


def targets_of_arena(recs: np.ndarray, offs, refs, **kw) -> Result:
    """The same over a record arena (offs: the record starts)."""
    out = []
    for o in offs:
        (bs,) = struct.unpack_from("<I", recs, int(o))
        out.append(recs[int(o):int(o) + 4 + bs].tobytes())
    return targets(out, refs, **kw)
