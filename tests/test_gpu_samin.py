"""GPU: SAM text parsed into BAM records on the device (csrc/sam_parse.hip: oge_sam_lines_dev, oge_sam_size_dev,
oge_sam_emit_dev, oge_sam_host_record, oge_sam_parse, the SAM branch of the module chain's FileReader and of
stats / count / coverage) equals the Python model (tests/samin_model.py) on every crafted case and on the SAM text of
the two real files, and the commands give the same records from x.sam as from x.bam.

None of the symbols exists before this feature, and `openge view x.sam` fails with "error reading": every test here
fails without it."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import bamutil
import sam_model
import samin_cases as K
import samin_model as M
from goldens import GOLDEN
from openge_amd import lib as L
from test_gpu_cli import OPENGE
from test_realign import load_rl_case

pytestmark = pytest.mark.gpu

CASES = K.cases()
ERRORS = K.error_cases()
CANARY = 64
FILES = {"simple": "simple.bam", "yhet208": "208.yhet.bam"}
# the model's field -> what the library's message says
SAYS = {"short": "shorter than 10", "fields": "fewer than 11 fields", "QNAME": "QNAME", "FLAG": "FLAG", "POS": "POS", "MAPQ": "MAPQ",
        "CIGAR": "CIGAR is not", "CIGAR ops": "more than 65535", "PNEXT": "PNEXT", "TLEN": "TLEN", "QUAL": "QUAL", "tag": "not shaped XX:T:",
        "tag type": "type outside AifZHB", "tag integer": "integer tag", "RNAME": "Rname nowhere missing from sequence dictionary"}


@functools.lru_cache(maxsize=None)
def file_text(name) -> tuple[bytes, tuple, tuple]:
    """(the SAM text of a real file by tests/sam_model.py, its contig names, its records), computed once."""
    htext, refs, recs, offs = bamutil.read_bam(GOLDEN / "inputs" / FILES[name])
    names = [n for n, _ in refs]
    records = sam_model.split_records(recs, offs)
    return htext.encode() + b"".join(sam_model.sam_line(r, names) for r in records), tuple(names), tuple(records)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(records, warning flags, host flags, line offsets) of a crafted case by the model, computed once."""
    return (*M.parse_text(CASES[name]), M.line_offsets(CASES[name]))


def dev_text(text: bytes):
    return torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda() if text else torch.zeros(4, dtype=torch.uint8, device="cuda")


class Parsed:
    """The three device passes over one text; the arena is prefilled with 0xAA and carries a canary."""

    def __init__(self, ctx, text: bytes, names=None):
        self.text = text
        self.hl, self.header_lines = L.Context.sam_header(text)
        self.opts, self.keep = L.text_opts(M.contigs(text[:self.hl]) if names is None else list(names))
        self.d_text = dev_text(text)
        self.n = ctx.sam_lines_dev(self.d_text.data_ptr(), len(text), self.hl)
        self.d_lo = torch.full((self.n + 1,), -1, dtype=torch.int64, device="cuda")
        self.d_ro = torch.full((self.n + 1,), -1, dtype=torch.int64, device="cuda")
        self.d_mark = torch.full((max(self.n, 1),), 7, dtype=torch.uint8, device="cuda")
        self.d_warn = torch.full((max(self.n, 1),), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # the fills run on torch's stream, the library on the context's
        assert ctx.sam_lines_dev(self.d_text.data_ptr(), len(text), self.hl, self.d_lo.data_ptr(), self.n + 1) == self.n
        self.lo = self.d_lo.cpu().numpy().view(np.uint64)

    def size(self, ctx):
        self.total, self.n_host = ctx.sam_size_dev(self.d_text.data_ptr(), self.d_lo.data_ptr(), self.n, self.opts, self.d_ro.data_ptr(),
                                                   self.d_mark.data_ptr(), self.d_warn.data_ptr())
        self.ro = self.d_ro.cpu().numpy().view(np.uint64)
        self.mark = self.d_mark.cpu().numpy()[:self.n].tolist()
        self.warn = self.d_warn.cpu().numpy()[:self.n].tolist()
        return self

    def emit(self, ctx, first, count):
        """The range's arena bytes as the device left them, the canary behind them checked."""
        nbytes = int(self.ro[first + count] - self.ro[first])
        out = torch.full((nbytes + CANARY,), 0xAA, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.sam_emit_dev(self.d_text.data_ptr(), self.d_lo.data_ptr(), self.d_ro.data_ptr(), first, count, self.opts, out.data_ptr(), nbytes)
        ctx.sync()
        h = out.cpu().numpy()
        assert (h[nbytes:] == 0xAA).all(), "bytes behind the range's records were written"
        return h[:nbytes].tobytes()

    def line(self, i) -> bytes:
        return self.text[int(self.lo[i]):int(self.lo[i + 1]) - 1]


def check_against(ctx, p: Parsed, recs, warns, hosts, loff):
    n = len(recs)
    assert p.n == n and p.lo.tolist() == loff
    p.size(ctx)
    assert np.array_equal(np.diff(p.ro), np.array([len(r) for r in recs], np.uint64)) and p.ro[0] == 0 and p.total == sum(map(len, recs))
    assert p.mark == [int(h) for h in hosts] and p.warn == [int(w) for w in warns]
    assert p.n_host == sum(hosts) and ctx.counter("sam_host_lines") == sum(hosts)
    whole = p.emit(ctx, 0, n)
    got = bytearray(whole)
    for i, h in enumerate(hosts):
        a, z = int(p.ro[i]), int(p.ro[i + 1])
        if h:  # the host's record goes over what the device left there
            got[a:z] = L.Context.sam_host_record(p.line(i), p.opts)
        assert bytes(got[a:z]) == recs[i], f"line {i}"
    return whole


@pytest.mark.parametrize("name", list(CASES))
def test_lines_size_and_emit_equal_the_model(ctx, name):
    """Line offsets, record offsets, host marks, warning bytes and record bytes per line; the marked set is the model's
    set of lines with an f or B tag, so the device cannot pass by handing its lines to the host; the emit pass in two
    ranges, cut at line 1, at n - 1, in the middle and around every marked line, stores what one range stores; and the
    host-buffer form returns the same records."""
    recs, warns, hosts, loff = expected(name)
    n = len(recs)
    p = Parsed(ctx, CASES[name])
    whole = check_against(ctx, p, recs, warns, hosts, loff)
    cuts = {1, n - 1, n // 2} | {i + d for i, h in enumerate(hosts) if h for d in (0, 1)}
    for c in sorted(x for x in cuts if 0 < x < n)[:8]:
        a = int(p.ro[c])
        assert p.emit(ctx, 0, c) == whole[:a] and p.emit(ctx, c, n - c) == whole[a:], c
    hl, r2, o2, w2 = ctx.sam_parse(CASES[name])
    assert hl == loff[0] and o2.tolist() == p.ro.tolist() and w2.tolist() == [int(w) for w in warns]
    assert r2[:p.total].tobytes() == b"".join(recs) and ctx.counter("sam_host_lines") == sum(hosts)


@pytest.mark.parametrize("name", sorted(FILES))
def test_real_files_are_parsed_on_the_device_alone(ctx, name):
    """Z and i tags only: no line may go to the host, and the records are the file's own, bin and tag types included."""
    text, names, records = file_text(name)
    p = Parsed(ctx, text, names)
    check_against(ctx, p, list(records), [0] * len(records), [0] * len(records), M.line_offsets(text))
    assert p.n_host == 0 and not any(p.mark)
    hl, r2, o2, _w = ctx.sam_parse(text)
    assert r2[:int(o2[-1])].tobytes() == b"".join(records) and ctx.counter("sam_host_lines") == 0


def test_simple_sam_is_simple_bam(ctx):
    _t, _r, recs, offs = bamutil.read_bam(GOLDEN / "inputs" / "simple.bam")
    hl, r2, o2, w2 = ctx.sam_parse((GOLDEN / "inputs" / "simple.sam").read_bytes())
    assert r2[:int(o2[-1])].tobytes() == recs.tobytes() and o2[:-1].tolist() == offs.tolist() and not w2.any()


def test_kernel_geometry_is_what_the_cases_assume(ctx):
    p = Parsed(ctx, CASES["basic_5"])
    assert ctx.timing("sam_lines") > 0
    p.size(ctx)
    assert (ctx.counter("sam_wave_lines"), ctx.counter("sam_block_lines")) == (K.WAVE_LINES, K.BLOCK_LINES)
    assert ctx.timing("sam_size") > 0
    p.emit(ctx, 0, p.n)
    assert ctx.timing("sam_emit") > 0


def test_a_changed_contig_table(ctx):
    """The same lines against other tables: refIDs follow the table of the call, no contigs at all refuses the RNAME."""
    body = b"\n".join([K.line("a", rname="c", rnext="chr2", flag=1), K.line("b", rname="chr2", rnext="=", flag=1), K.line("u", rname="*", rnext="zz")]) + b"\n"
    for names in (["c", "chr2"], ["chr2", "c"], ["x", "zz", "c", "chr2"], ["c", "chr2"]):
        want, warns, hosts = M.parse_text(body, names)
        p = Parsed(ctx, body, names).size(ctx)
        assert p.emit(ctx, 0, p.n) == b"".join(want) and p.warn == [int(w) for w in warns], names
    with pytest.raises(L.OgeError, match="error -1: Rname c missing from sequence dictionary .*line 1:"):
        Parsed(ctx, body, []).size(ctx)


@pytest.mark.parametrize("name", list(ERRORS))
def test_errors_name_the_line_and_nothing_is_handed_on(ctx, name):
    text, line, field = ERRORS[name]
    p = Parsed(ctx, text)
    with pytest.raises(L.OgeError) as e:
        p.size(ctx)
    assert "error -1: " in str(e.value) and f"line {line}: " in str(e.value) and SAYS[field] in str(e.value), str(e.value)
    assert ctx.counter("sam_bad_line") == line
    # the caller's arrays are as they were before the call
    assert (p.d_ro.cpu().numpy() == -1).all() and (p.d_mark.cpu().numpy() == 7).all() and (p.d_warn.cpu().numpy() == 7).all()
    hl, nb, n = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
    recs, offs, warn = C.c_void_p(1), C.c_void_p(1), C.c_void_p(1)
    rc = L.lib().oge_sam_parse(ctx.h, text, len(text), C.byref(hl), C.byref(recs), C.byref(nb), C.byref(offs), C.byref(n), C.byref(warn))
    assert rc == -1 and f"line {line}: ".encode() in L.lib().oge_last_error(ctx.h)
    assert (recs.value, offs.value, warn.value, nb.value, n.value) == (None, None, None, 0, 0)
    with pytest.raises(L.OgeError, match="error -1: sam: "):
        L.Context.sam_host_record(M.split_text(text)[1][line - 1 - p.header_lines], p.opts)


def test_a_host_line_that_does_not_parse(ctx):
    """The size pass takes an f tag as 7 bytes whatever its value; the host names the line."""
    lines = [K.basic(i) for i in range(5)]
    lines[3] = K.line("f", tags=("XF:f:1.5x",))
    at = K.header().count(b"\n") + 4
    with pytest.raises(L.OgeError, match=rf"error -1: sam: line {at}: .*XF"):
        ctx.sam_parse(K.text(lines))
    lines[3] = K.line("b", tags=("XB:B:c,1,128",))
    with pytest.raises(L.OgeError, match=rf"error -1: sam: line {at}: .*XB"):
        ctx.sam_parse(K.text(lines))


def test_argument_errors_and_the_small_buffer(ctx):
    p = Parsed(ctx, CASES["basic_5"]).size(ctx)
    lib = L.lib()
    out = torch.full((p.total + CANARY,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    args = (ctx.h, p.d_text.data_ptr(), p.d_lo.data_ptr(), p.d_ro.data_ptr(), 0, p.n, C.byref(p.opts), out.data_ptr())
    assert lib.oge_sam_emit_dev(*args, p.total - 1) == -3 and b"smaller" in lib.oge_last_error(ctx.h)
    ctx.sync()
    assert (out.cpu().numpy() == 0xAA).all()
    assert lib.oge_sam_emit_dev(*args, p.total) == 0
    tot, nh, n = C.c_uint64(), C.c_uint64(), C.c_uint64()
    t = p.d_text.data_ptr()
    assert lib.oge_sam_size_dev(ctx.h, t, p.d_lo.data_ptr(), 1, None, p.d_ro.data_ptr(), t, t, C.byref(tot), C.byref(nh)) == -1
    assert b"null argument" in lib.oge_last_error(ctx.h)
    assert lib.oge_sam_size_dev(ctx.h, t, p.d_lo.data_ptr(), (1 << 32) - 1, C.byref(p.opts), p.d_ro.data_ptr(), t, t, C.byref(tot), C.byref(nh)) == -3
    assert b"2^32" in lib.oge_last_error(ctx.h)
    assert lib.oge_sam_lines_dev(ctx.h, t, len(p.text), len(p.text) + 1, None, 0, C.byref(n)) == -1
    assert lib.oge_sam_lines_dev(ctx.h, t + 1, len(p.text) - 1, 0, None, 0, C.byref(n)) == -1 and b"aligned" in lib.oge_last_error(ctx.h)
    assert lib.oge_sam_lines_dev(ctx.h, t, len(p.text), p.hl, p.d_lo.data_ptr(), p.n, C.byref(n)) == -3 and n.value == p.n
    # a header the header model refuses (an @SQ line without LN) is refused here as the commands refuse it
    with pytest.raises(L.OgeError, match="error -1: sam: header: Mandatory field missing in header sequence line"):
        ctx.sam_parse(b"@SQ\tSN:c\n" + K.line("a") + b"\n")
    buf = C.create_string_buffer(8)
    ln = C.c_uint64()
    assert lib.oge_sam_host_record(p.line(0), len(p.line(0)), C.byref(p.opts), buf, 8, C.byref(ln)) == -3 and ln.value == int(p.ro[1])


# ------------------------------------------------------------------------------------------------ the CLI
def cli(*args, env=None, stdin=None):
    return subprocess.run([OPENGE, *map(str, args)], capture_output=True, timeout=300, env={**os.environ, **(env or {})}, input=stdin)


def records_of(path) -> list[bytes]:
    _t, _r, recs, offs = bamutil.read_bam(path)
    return sam_model.split_records(recs, offs)


@pytest.fixture(scope="module")
def sams(tmp_path_factory, built):
    """x.sam beside x.bam for the two files: the text `openge view --nopg` writes of the BAM file."""
    d = tmp_path_factory.mktemp("samin")
    out = {}
    for name, fn in FILES.items():
        r = cli("view", "--nopg", GOLDEN / "inputs" / fn)
        assert r.returncode == 0, r.stderr
        (d / f"{name}.sam").write_bytes(r.stdout)
        out[name] = (d / f"{name}.sam", GOLDEN / "inputs" / fn)
    return out


def test_cli_view_of_sam_is_the_identity(sams, tmp_path):
    """`view simple.sam` prints the file's own text, `view -F bam in.sam | view` too, and both take the device path."""
    fixture = GOLDEN / "inputs" / "simple.sam"
    r = cli("view", "--nopg", fixture)
    assert r.returncode == 0 and r.stdout == fixture.read_bytes(), r.stderr
    for name, (sam, _bam) in sams.items():
        r = cli("view", "--nopg", "-v", sam)
        assert r.returncode == 0 and r.stdout == sam.read_bytes(), r.stderr
        assert b" 0 lines built on the host" in r.stderr
        st = cli("view", "--nopg", sam, env={"OGE_STREAM_MIN": "1"})  # the streamed file-to-HBM loader
        assert st.returncode == 0 and st.stdout == r.stdout, st.stderr
        mid = tmp_path / f"{name}.bam"
        assert cli("view", "--nopg", "-F", "bam", "-o", mid, sam).returncode == 0
        back = cli("view", "--nopg", mid)
        assert back.returncode == 0 and back.stdout == sam.read_bytes()


@pytest.mark.parametrize("name", sorted(FILES))
@pytest.mark.parametrize("cmd", [("mergesort",), ("mergesort", "-M"), ("dedup",), ("sort", "-b")], ids=lambda c: "_".join(c))
def test_cli_commands_give_the_same_records_from_sam_as_from_bam(sams, cmd, name, tmp_path):
    sam, bam = sams[name]
    a, b = tmp_path / "from_sam.bam", tmp_path / "from_bam.bam"
    ra, rb = cli(*cmd, "--nopg", "-o", a, sam), cli(*cmd, "--nopg", "-o", b, bam)
    assert ra.returncode == 0 and rb.returncode == 0, (ra.stderr, rb.stderr)
    got, want = bamutil.read_bam(a), bamutil.read_bam(b)
    assert got[0] == want[0] and got[1] == want[1] and got[2].tobytes() == want[2].tobytes() and len(got[3]) == len(want[3]) > 0


def test_cli_merge_of_bam_and_sam_inputs_and_stdin(sams, tmp_path):
    """The reference's own test: simple.bam simple.bam simple.sam sorted together; SAM on stdin; two ranks."""
    fixture, bam = GOLDEN / "inputs" / "simple.sam", GOLDEN / "inputs" / "simple.bam"
    a, b = tmp_path / "a.bam", tmp_path / "b.bam"
    assert cli("mergesort", "--nopg", "-o", a, bam, bam, fixture).returncode == 0
    assert cli("mergesort", "--nopg", "-o", b, bam, bam, bam).returncode == 0
    assert records_of(a) == records_of(b) and len(records_of(a)) == 3 * len(records_of(bam))
    for cmd in (("mergesort",), ("view", "-F", "bam")):
        c = tmp_path / "c.bam"
        assert cli(*cmd, "--nopg", "-o", c, stdin=fixture.read_bytes()).returncode == 0
        assert cli(*cmd, "--nopg", "-o", b, bam).returncode == 0
        assert records_of(c) == records_of(b)
    sam, ybam = sams["yhet208"]
    ra, rb = cli("mergesort", "--nopg", "--gpus", "2", "-o", a, sam), cli("mergesort", "--nopg", "--gpus", "2", "-o", b, ybam)
    assert ra.returncode == 0 and rb.returncode == 0, (ra.stderr, rb.stderr)
    assert records_of(a) == records_of(b)


@pytest.mark.parametrize("name", sorted(FILES))
def test_cli_count_stats_and_coverage_of_sam(sams, name, tmp_path):
    sam, bam = sams[name]
    for args in (("count",), ("stats", "-I", "-L")):
        ra, rb = cli(*args, sam), cli(*args, bam)
        assert ra.returncode == 0 and rb.returncode == 0 and ra.stdout == rb.stdout != b"", (ra.stderr, rb.stderr)
    ra, rb = cli("coverage", "-b", "1000", "-o", tmp_path / "a.tsv", sam), cli("coverage", "-b", "1000", "-o", tmp_path / "b.tsv", bam)
    assert ra.returncode == 0 and rb.returncode == 0 and ra.stderr == rb.stderr, (ra.stderr, rb.stderr)
    assert (tmp_path / "a.tsv").read_bytes() == (tmp_path / "b.tsv").read_bytes() != b""


def test_cli_host_lines_and_warnings(tmp_path):
    """f and B tags through the commands: the records are the model's; an unknown RNEXT warns as the reference does."""
    for name in ("host_tags", "rnext", "mix"):
        src = tmp_path / f"{name}.sam"
        src.write_bytes(CASES[name])
        out = tmp_path / f"{name}.bam"
        r = cli("view", "--nopg", "-F", "bam", "-o", out, src)
        assert r.returncode == 0, r.stderr
        recs, warns, _h = M.parse_text(CASES[name])
        assert records_of(out) == recs
        said = [ln for ln in r.stderr.decode().splitlines() if ln.startswith("RNext ")]
        want = ["RNext " + ln.split(b"\t")[6].decode() + " missing from sequence dictionary" for ln, w in zip(M.split_text(CASES[name])[1], warns) if w]
        assert said == want
    # more marked lines than are fetched one by one: the whole text comes down once, runs of records go up
    many = K.text([K.basic(i) if i % 3 == 0 else K.line(f"f{i}", tags=("XF:f:0.5", f"XB:B:s,{i},-1")) for i in range(6300)])
    (tmp_path / "many.sam").write_bytes(many)
    r = cli("view", "--nopg", "-v", "-F", "bam", "-o", tmp_path / "many.bam", tmp_path / "many.sam")
    assert r.returncode == 0 and b" 4200 lines built on the host" in r.stderr, r.stderr
    assert records_of(tmp_path / "many.bam") == M.parse_text(many)[0]
    r = cli("view", "--nopg", "-F", "bam", "-o", tmp_path / "s.bam", stdin=CASES["rnext"])
    assert r.returncode == 0 and records_of(tmp_path / "s.bam") == M.parse_text(CASES["rnext"])[0]
    assert r.stderr.decode().count("missing from sequence dictionary") == sum(M.parse_text(CASES["rnext"])[1])


def test_cli_refusals(tmp_path):
    """An unknown RNAME exits -1 with the reference's line; a bad line fails before any output file exists, from a file
    and from stdin; `index` refuses SAM."""
    text, line, _f = ERRORS["rname_unknown_middle"]
    src = tmp_path / "bad.sam"
    src.write_bytes(text)
    for kw in ({"args": (src,)}, {"args": (), "stdin": text}):
        out = tmp_path / "out.bam"
        r = cli("mergesort", "-o", out, *kw["args"], stdin=kw.get("stdin"))
        assert r.returncode == 255 and r.stderr.decode().splitlines()[0] == "Rname nowhere missing from sequence dictionary", r.stderr
        assert f"line {line}".encode() in r.stderr and not out.exists() and r.stdout == b""
    text, line, _f = ERRORS["flag_text_last"]
    src.write_bytes(text)
    for cmd in (("view", "-F", "bam"), ("dedup",), ("sort",)):
        out = tmp_path / "o.bam"
        r = cli(*cmd, "-o", out, src)
        assert r.returncode != 0 and f"line {line}: FLAG".encode() in r.stderr and not out.exists() and r.stdout == b"", r.stderr
    for cmd in (("count",), ("stats",), ("coverage",)):
        r = cli(*cmd, src)
        assert r.returncode != 0 and f"line {line}: FLAG".encode() in r.stderr and r.stdout == b""
    src.write_bytes(CASES["basic_5"])
    r = cli("index", src)
    assert r.returncode != 0 and b"is SAM text" in r.stderr and not (tmp_path / "bad.sam.bai").exists()


def test_cli_localrealign_of_sam(tmp_path):
    """localrealign reads x.sam through the same FileReader: the realigned reads are those from x.bam.  They are
    compared as SAM text: this input's BAM stores small integer tags in wider types than SAM input chooses (the
    reference's smallest-type rule), a width that SAM text cannot carry."""
    _meta, _arrays, _h, _recs, _offs, fa, iv = load_rl_case("rl_small", tmp_path)
    bam, sam = tmp_path / "reads.bam", tmp_path / "reads.sam"
    v = cli("view", "--nopg", "-o", sam, bam)
    assert v.returncode == 0 and sam.read_bytes()[:1] == b"@", v.stderr
    a, b = tmp_path / "from_sam.bam", tmp_path / "from_bam.bam"
    ra = cli("localrealign", "--nopg", "-R", fa, "-L", iv, sam, "-o", a)
    rb = cli("localrealign", "--nopg", "-R", fa, "-L", iv, bam, "-o", b)
    assert ra.returncode == 0 and rb.returncode == 0, (ra.stderr, rb.stderr)
    got, want = bamutil.read_bam(a), bamutil.read_bam(b)
    names = [n for n, _ in want[1]]
    text = [sam_model.lines(sam_model.split_records(x[2], x[3]), names) for x in (got, want)]
    assert got[0] == want[0] and got[1] == want[1] and text[0] == text[1] and len(text[1]) > 0
    assert len(got[2]) < len(want[2])  # the narrower tags are the only difference
