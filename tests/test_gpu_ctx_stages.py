"""GPU: what a context reports about its last call (oge_ctx_timing, oge_ctx_counter) after a call that failed
and after a composite call that succeeded.

A stage is timed by an OgeStage and a composite entry point holds its sub-calls' stages and counters with an
OgeCall (csrc/oge_ctx.h): both close at the end of their scope, so an error return in the middle of a stage
leaves a stage whose stop event was recorded and a hold that came back down.  The failing input is the one of
test_record_offsets_reject_bad_block_size: a handled error return of the record walk."""
import functools
import struct

import numpy as np
import pytest
import torch

import qc_cases as K
from goldens import GOLDEN
from openge_amd import lib as L
from test_gpu_inflate import _stream, bgzf

pytestmark = pytest.mark.gpu

CHAIN_STAGES = ("bgzf_index", "bgzf_inflate", "rec_walk")  # the reader half every whole-file entry point runs


@functools.lru_cache(maxsize=None)
def bad_stream():
    """(a decompressed BAM stream whose middle record has block_size 20000, the start of its records, n_ref)"""
    raw, base, n_ref, want = _stream(40_000, 4)
    bad = bytearray(raw)
    struct.pack_into("<I", bad, int(want[len(want) // 2]), 20000)  # > 10000 (bam_deserializer.h:160-163)
    return bytes(bad), base, n_ref


@pytest.fixture
def failed_ctx(ctx):
    """A fresh context whose only call so far, bam_count of the bad stream's file, failed in the record walk."""
    bad, base, n_ref = bad_stream()
    d = torch.frombuffer(bytearray(bad + bytes(64)), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    with pytest.raises(L.OgeError):
        ctx.record_offsets_dev(d.data_ptr(), base, len(bad), n_ref)
    ctx2 = L.Context(0)
    try:
        with pytest.raises(L.OgeError):
            ctx2.bam_count(bgzf(bad, 1))
        yield ctx2
    finally:
        ctx2.close()


def test_failed_call_leaves_its_stages_readable(failed_ctx):
    """The record walk returned an error between its stage's start and end: the stage still has its stop event,
    so the timing query answers instead of failing on an event that was never recorded."""
    for name in CHAIN_STAGES:
        assert failed_ctx.timing(name) >= 0, name


def test_hold_comes_back_down_after_a_failure(failed_ctx):
    """bam_count held the stages and counters of its sub-calls; after its failure a plain call starts from
    nothing again: the counter an earlier call set is gone, and the call's own stage is there."""
    recs, offs = K.pack([K.rec(0, 0, 5), K.rec(1, 3, 5)])
    d_recs = torch.from_numpy(np.ascontiguousarray(recs)).cuda()
    d_off = torch.from_numpy(np.asarray(offs, np.uint64).view(np.int64).copy()).cuda()
    d_toff = torch.zeros(3, dtype=torch.int64, device="cuda")
    d_mark = torch.zeros(2, dtype=torch.uint8, device="cuda")
    opts, _keep = L.text_opts(["c", "d"])
    torch.cuda.synchronize()  # the fills run on torch's stream, the library on the context's
    total, n_host = failed_ctx.text_size_dev(d_recs.data_ptr(), d_off.data_ptr(), 2, opts, d_toff.data_ptr(), d_mark.data_ptr())
    assert total > 0 and n_host == 0
    out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    failed_ctx.text_emit_dev(d_recs.data_ptr(), d_off.data_ptr(), d_toff.data_ptr(), 0, 2, opts, out.data_ptr(), total)
    assert failed_ctx.counter("text_wave_records") is not None
    failed_ctx.stats_dev(d_recs.data_ptr(), d_off.data_ptr(), 2)
    assert failed_ctx.counter("text_wave_records") is None
    assert failed_ctx.timing("qc_stats") >= 0


def test_composite_call_reports_every_stage(ctx):
    assert ctx.bam_count((GOLDEN / "inputs" / "simple.bam").read_bytes()) > 0
    for name in CHAIN_STAGES:
        assert ctx.timing(name) >= 0, name  # -1: the stage is absent
    assert ctx.timing("no_such_stage") == -1
