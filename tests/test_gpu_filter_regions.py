"""Region lists on the GPU (oge_filter_regions_dev; view / mergesort / sort -L) against the plain-Python
predicate of regions_model, and against the single-region filter where the two must agree byte for byte."""
import random
import subprocess

import numpy as np
import pytest
import torch

import bamutil
import regions_model as R
from goldens import load_case
from openge_amd import lib as L
from test_gpu_cli import OPENGE, case_input
from test_regions_model import random_regions

pytestmark = pytest.mark.gpu
N_REF = 4


@pytest.fixture(scope="module")
def records():
    """3,000 records over 4 contigs and refID -1, positions 0..3000 so that random regions of that range keep
    some and drop some; l_seq 0..150; a few ends that wrap past 2^31 - 1."""
    rng = random.Random(5)
    out = []
    for i in range(3000):
        refid = rng.choice([-1, 0, 1, 2, 3])
        pos = rng.randrange(0, 3000) if i % 97 else (1 << 31) - 1 - rng.randrange(0, 50)
        lseq = rng.choice([0, 1, 36, 100, rng.randrange(0, 150)])
        out.append(bamutil.make_record(f"r{i}", 0, refid, pos if refid >= 0 else -1, f"{lseq}M" if lseq else "", "A" * lseq,
                                       mapq=rng.randrange(0, 61)))
    return out


WHOLE = [(r, -(1 << 31), (1 << 31) - 1) for r in (-1, 0, 1, 2, 3)]


@pytest.fixture(scope="module")
def out_form(ctx, records):
    """Every record as the filter writes it (the gather recomputes the bin): from a list of whole contigs, which
    keeps all but the empty reads (l_seq > trim total is part of the predicate) -- those never appear."""
    out, oo = dev_filter(ctx, records, WHOLE)
    keep = R.keep_regions(records, WHOLE)
    assert len(oo) - 1 == len(keep) and set(keep) == {i for i, rb in enumerate(records) if R.core(rb)[3] > 0}
    return {i: out[oo[k]:oo[k + 1]] for k, i in enumerate(keep)}


def dev_filter(ctx, records, regions, single=False, **kw):
    recs, offs = bamutil.pack_records(records)
    n = len(records)
    d_recs = torch.from_numpy(recs).cuda()
    d_off = torch.from_numpy(offs.view(np.int64)).cuda()
    d_out = torch.zeros(int(offs[n]) + 64, dtype=torch.uint8, device="cuda")
    d_oo = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    if single:
        (ref, left, right), = regions
        m = ctx.filter_records_dev(d_recs.data_ptr(), d_off.data_ptr(), n,
                                   L.filter_opts(has_region=1, ref_id=ref, left_pos=left, right_pos=right, **kw),
                                   d_out.data_ptr(), d_oo.data_ptr())
    else:
        m = ctx.filter_regions_dev(d_recs.data_ptr(), d_off.data_ptr(), n, L.filter_opts(**kw), regions, d_out.data_ptr(),
                                   d_oo.data_ptr())
    ctx.sync()
    oo = d_oo.cpu().numpy().view(np.uint64)[:m + 1]
    return d_out.cpu().numpy()[:int(oo[m])].tobytes(), [int(x) for x in oo]


# 1, 2: the smallest lists; 63, 64, 65: one wave of the key kernel and its neighbours; 300, 1000: more than one
# workgroup of the key kernels and more than one 256-entry step (with its carry) of the running maximum
@pytest.mark.parametrize("n_regions", [1, 2, 63, 64, 65, 300, 1000])
def test_list_equals_the_python_predicate(ctx, records, out_form, n_regions):
    # seeds of the two smallest lists chosen so that they keep something: one region, two touching ones
    regions = random_regions(random.Random({1: 105, 2: 111}.get(n_regions, n_regions)), n_regions, N_REF)
    got, oo = dev_filter(ctx, records, regions)
    keep = R.keep_regions(records, regions)
    assert 0 < len(keep) < len(records)
    assert len(oo) - 1 == len(keep)
    assert got == b"".join(out_form[i] for i in keep)


@pytest.mark.parametrize("kw", [dict(count_limit=1), dict(count_limit=17), dict(count_limit=0), dict(mapq_min=30, count_limit=40),
                                dict(min_len=30, max_len=100), dict(trim_total=36)])
def test_other_settings_apply_as_with_one_region(ctx, records, out_form, kw):
    regions = random_regions(random.Random(11), 65, N_REF)
    got, oo = dev_filter(ctx, records, regions, **kw)
    keep = R.keep_regions(records, regions, **kw)
    assert len(oo) - 1 == len(keep)
    assert got == b"".join(out_form[i] for i in keep)


@pytest.mark.parametrize("region", [(0, 100, 2000), (2, 1000, 1000), (1, 1500, 1480), (-1, -5, 5), (7, 0, 100), (3, 2999, (1 << 31) - 1)])
@pytest.mark.parametrize("kw", [dict(), dict(count_limit=5, mapq_min=20)])
def test_one_region_equals_the_single_region_filter_byte_for_byte(ctx, records, region, kw):
    a = dev_filter(ctx, records, [region], **kw)
    b = dev_filter(ctx, records, [region], single=True, **kw)
    assert a == b
    assert len(a[1]) - 1 == len(R.keep_regions(records, [region], **kw))


def test_zero_records_and_no_region(ctx, records):
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    oo = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    assert ctx.filter_regions_dev(d.data_ptr(), oo.data_ptr(), 0, L.filter_opts(), [(0, 0, 10)], d.data_ptr(), oo.data_ptr()) == 0
    ctx.sync()
    assert int(oo[0]) == 0
    with pytest.raises(L.OgeError, match="no region"):
        ctx.filter_regions_dev(d.data_ptr(), oo.data_ptr(), 0, L.filter_opts(), [], d.data_ptr(), oo.data_ptr())


# ------------------------------------------------------------------------------------------ the CLI
def cli(*args):
    return subprocess.run([OPENGE, *map(str, args)], capture_output=True, timeout=300)


@pytest.fixture(scope="module")
def c2(tmp_path_factory, built):
    tmp = tmp_path_factory.mktemp("regions")
    src = case_input(load_case("c2_20k"), tmp)
    _h, refs, recs, offs = bamutil.read_bam(src)
    records = [bamutil.rec_bytes(recs, o) for o in offs]
    rng = random.Random(3)
    used = sorted({R.core(rb)[0] for rb in records if R.core(rb)[0] >= 0})
    lines, regions = ["# regions of the test", ""], []
    for k in range(40):
        ref = rng.choice(used)
        ps = [R.core(rb)[1] for rb in records if R.core(rb)[0] == ref]
        a = rng.choice(ps)
        b = min(a + rng.randrange(0, 200_000), refs[ref][1])
        if k % 3 == 0:
            lines.append(f"{refs[ref][0]}:{a}")
            regions.append((ref, a, a))
        else:
            lines.append(f"{refs[ref][0]}:{a}..{b}")
            regions.append((ref, a, b))
        if k % 10 == 0:
            lines.append("")
    lines.append(refs[used[-1]][0])  # a whole contig
    regions.append((used[-1], 0, refs[used[-1]][1]))
    path = tmp / "regions.txt"
    path.write_text("\n".join(lines) + "\n")
    return dict(tmp=tmp, src=src, refs=refs, records=records, regions=regions, file=path)


def same_records(path, records, keep):
    _h, _r, recs, offs = bamutil.read_bam(path)
    got = [bamutil.match_key(bamutil.rec_bytes(recs, o)) for o in offs]
    assert got == [bamutil.match_key(records[i]) for i in keep]


def test_cli_view_L_equals_the_python_predicate(c2):
    keep = R.keep_regions(c2["records"], c2["regions"])
    assert 0 < len(keep) < len(c2["records"])
    out = c2["tmp"] / "v.bam"
    r = cli("view", "--nopg", "-L", c2["file"], c2["src"], "-o", out)
    assert r.returncode == 0, r.stderr
    same_records(out, c2["records"], keep)
    # SAM text: the same reads in the same order
    r = cli("view", "--nopg", "-L", c2["file"], c2["src"])
    assert r.returncode == 0, r.stderr
    body = [ln.split("\t") for ln in r.stdout.decode().splitlines() if not ln.startswith("@")]
    assert [(f[0], int(f[3]) - 1) for f in body] == [(bamutil.fields(c2["records"][i])["name"], R.core(c2["records"][i])[1]) for i in keep]


def test_cli_view_L_with_r_n_and_q(c2):
    ref, a, b = c2["regions"][1]
    extra = (c2["regions"][5][0], 0, 50_000)
    name = c2["refs"][extra[0]][0]
    out = c2["tmp"] / "u.bam"
    r = cli("view", "--nopg", "-L", c2["file"], "-r", f"{name}:0..50000", "-q", 20, "-n", 300, c2["src"], "-o", out)
    assert r.returncode == 0, r.stderr
    keep = R.keep_regions(c2["records"], [extra] + c2["regions"], mapq_min=20, count_limit=300)
    assert len(keep) == 300
    same_records(out, c2["records"], keep)


def test_cli_one_line_list_equals_r(c2):
    ref, a, b = c2["regions"][1]
    one = c2["tmp"] / "one.txt"
    one.write_text(f"#c\n{c2['refs'][ref][0]}:{a}..{b}\n")
    x = cli("view", "--nopg", "-L", one, c2["src"])
    y = cli("view", "--nopg", "-r", f"{c2['refs'][ref][0]}:{a}..{b}", c2["src"])
    assert x.returncode == 0 and y.returncode == 0
    assert x.stdout == y.stdout and x.stdout.count(b"\n") > 10


def test_cli_sort_L_equals_sort_of_the_kept_reads(c2):
    keep = R.keep_regions(c2["records"], c2["regions"])
    h, refs, _r, _o = bamutil.read_bam(c2["src"])
    pre = c2["tmp"] / "pre.bam"
    bamutil.write_bam_py(pre, h, refs, [c2["records"][i] for i in keep])
    a, b = c2["tmp"] / "a.bam", c2["tmp"] / "b.bam"
    assert cli("sort", "--nopg", "-L", c2["file"], c2["src"], "-o", a).returncode == 0
    assert cli("sort", "--nopg", pre, "-o", b).returncode == 0
    assert a.read_bytes() == b.read_bytes()


def test_cli_L_on_sam_input_and_on_two_inputs(c2):
    sam = c2["tmp"] / "in.sam"
    r = cli("view", "--nopg", c2["src"], "-o", sam)
    assert r.returncode == 0, r.stderr
    want = cli("view", "--nopg", "-L", c2["file"], c2["src"]).stdout
    got = cli("view", "--nopg", "-L", c2["file"], sam)
    assert got.returncode == 0, got.stderr
    assert got.stdout == want
    # two inputs through the ordinary reader: as many reads as the two lists together
    two = cli("mergesort", "--nopg", "-L", c2["file"], c2["src"], c2["src"], "-o", c2["tmp"] / "two.bam")
    assert two.returncode == 0, two.stderr
    _h, _r, _recs, offs = bamutil.read_bam(c2["tmp"] / "two.bam")
    assert len(offs) == 2 * len(R.keep_regions(c2["records"], c2["regions"]))


def test_cli_bad_line_names_its_line_number_and_writes_nothing(c2):
    bad = c2["tmp"] / "bad.txt"
    name = c2["refs"][0][0]
    bad.write_text(f"{name}:10..20\n\n# comment\nnot_a_contig:5\n{name}:7\n")
    out = c2["tmp"] / "never.bam"
    r = cli("view", "-L", bad, c2["src"], "-o", out)
    assert r.returncode != 0
    assert b"bad.txt line 4" in r.stderr and b"not_a_contig" in r.stderr
    assert not out.exists() or out.stat().st_size == 0
    r = cli("view", "-L", bad, c2["src"])
    assert r.returncode != 0 and r.stdout == b""
    # before anything is read: under -v no reader has reported a file -- BAM without an index, --noindex, SAM
    # text, several inputs, the sorting chain
    sam = c2["tmp"] / "bad_in.sam"
    assert cli("view", "--nopg", c2["src"], "-o", sam).returncode == 0
    for args in (("view", c2["src"]), ("view", "--noindex", c2["src"]), ("view", sam), ("mergesort", c2["src"], c2["src"]),
                 ("sort", c2["src"]), ("view", "-r", f"{name}:1..5", c2["src"])):
        r = cli(args[0], "-v", "-L", bad, *args[1:], "-o", out)
        assert r.returncode != 0 and b"bad.txt line 4" in r.stderr, args
        assert b"FileReader (" not in r.stderr and b"alignments processed" not in r.stderr, (args, r.stderr)
        assert not out.exists() or out.stat().st_size == 0
    good = cli("view", "-v", "-L", c2["file"], c2["src"], "-o", out)  # the line the checks above look for exists
    assert good.returncode == 0 and b"FileReader (" in good.stderr


def test_cli_unreadable_list_is_refused(c2):
    r = cli("view", "-L", c2["tmp"] / "missing.txt", c2["src"])
    assert r.returncode != 0 and b"cannot read the regions file" in r.stderr and r.stdout == b""
