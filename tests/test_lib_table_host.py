"""The read-group -> library table that the library builds from a BAM header (oge_bam_markdup_opts, the table of
every dedup chain and of the duplication metrics) equals the two independent constructions the tests use:
lib.markdup_opts_from_header and dupmetrics_model.lib_table.  Ids run from 1 in the order the names first appear, an
@RG without an LB is in "Unknown Library", unknown_lib is that name's id or else the next free one."""
import ctypes as C

import numpy as np
import pytest

import dupmetrics_cases as DK
import dupmetrics_model as DM
import markdup_wide_cases as W
from openge_amd import lib as L

HEADERS = {
    "rg_shapes": DK.rg_shapes()[0],
    "no_rg": DK.header_text([]),
    "one_rg_no_lb": DK.header_text([("g1", None)]),
    "unknown_spelled_and_absent": DK.header_text([("g1", "Unknown Library"), ("g2", None)]),
    "one_id_two_libraries": DK.header_text([("g1", "libA"), ("g1", "libB")]),
    "wide": W.make_header(1023, 3)[0],
}


def table_of(opts):
    """(id bytes, rg_lib[:n_rg], n_rg, unknown_lib) behind the pointers of a MarkdupOpts"""
    libs = np.ctypeslib.as_array((C.c_int16 * opts.n_rg).from_address(opts.rg_lib)).tolist() if opts.n_rg else []
    return C.string_at(opts.rg_ids, opts.rg_ids_bytes) if opts.rg_ids_bytes else b"", libs, opts.n_rg, opts.unknown_lib


@pytest.mark.parametrize("name", list(HEADERS))
def test_the_built_table_equals_both_constructions(built, tmp_path, name):
    header = HEADERS[name]
    path = tmp_path / "h.bam"
    L.write_bam(path, header, np.zeros(16, np.uint8), np.zeros(1, np.uint64), 0)
    bam = L.Bam(path)
    assert bam.n == 0 and bam.n_ref == header.count("@SQ\t")
    opts, keep = bam.markdup_opts()
    ids, libs, n_rg, unknown = table_of(opts)
    want, keep_want = L.markdup_opts_from_header(header, bam.n_ref)
    assert (ids, libs, n_rg, unknown) == table_of(want)
    assert n_rg == header.count("@RG\t") and opts.n_ref == bam.n_ref

    rg_lib, model_unknown, names = DM.lib_table(header)
    first = {}
    for rg_id, lib_id in zip(ids.split(b"\0")[:n_rg], libs):
        first.setdefault(rg_id, lib_id)  # the first read group of an id wins the lookup
    assert first == rg_lib and unknown == model_unknown
    assert 1 + max(libs + [unknown]) == len(names)


def test_the_shapes_the_headers_stand_for(built):
    """what the hand-written headers are there to show, on the independent construction"""
    o, keep = L.markdup_opts_from_header(HEADERS["no_rg"], 2)
    assert table_of(o) == (b"", [], 0, 1)
    o, keep = L.markdup_opts_from_header(HEADERS["one_rg_no_lb"], 2)
    assert table_of(o) == (b"g1\0", [1], 1, 1)
    o, keep = L.markdup_opts_from_header(HEADERS["unknown_spelled_and_absent"], 2)
    assert table_of(o) == (b"g1\0g2\0", [1, 1], 2, 1)
    o, keep = L.markdup_opts_from_header(HEADERS["one_id_two_libraries"], 2)
    assert table_of(o) == (b"g1\0g1\0", [1, 2], 2, 3)
    assert DM.lib_table(HEADERS["one_id_two_libraries"])[0] == {b"g1": 1}
