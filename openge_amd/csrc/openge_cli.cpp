// openge_cli.cpp -- the `openge` command-line drop-in for OpenGE's hot-path commands
// (oge/main.cpp:24-42, commands/commands.cpp:34-169): mergesort (+ the `sort` alias),
// dedup and localrealign, with the reference's option names and defaults.  Each command builds the
// same module chain the reference builds (commands/command_mergesort.cpp:68-117,
// command_dedup.cpp:48-69, command_localrealign.cpp:37-75) out of the modules in modules.h.
// `view` is FileReader -> Filter -> FileWriter (commands/command_view.cpp:44-100), SAM to stdout by default.
// -L FILE (view, mergesort, sort; not in the reference): a list of regions in the syntax of -r, one per line; a read
// is kept when it passes -r's test for at least one of them (and for -r's own region, when both are given).
// With regions and an index beside the one BAM input (in.bam.bai or in.bai, not older than the file) the reader takes only
// the blocks the index names (FileReader::read_indexed) and the input is not prefetched; anything
// wrong with the index gives the full scan, with one [openge] line under -v; --noindex never looks for an index.
// `index`, `stats`, `count` and `coverage` are one whole-file device call each (index_bam_file,
// stats_bam_file, count_bam_file, coverage_bam_file in modules.cpp; commands/command_stats.cpp,
// command_count.cpp, command_coverage.cpp for the last three).
// `compare` loads every input into HBM and takes the multiset difference of the read placements there
// (compare_files in modules.cpp, csrc/compare.hip; commands/command_compare.cpp).
// `targets` (not in the reference, whose comments send the user to GATK's RealignerTargetCreator) computes the
// intervals file localrealign -L takes from the reads' own indels (targets_bam_file, csrc/targets.hip; DESIGN.md
// section 25); `localrealign --auto-targets` computes the same intervals from the records it is handed.
// `dedup --metrics FILE` and `mergesort -M --metrics FILE` also write Picard MarkDuplicates' metrics file, which the
// reference never wrote (algorithms/mark_duplicates.cpp has no metrics code); `dupmetrics` writes it for a file that
// is already marked (dupmetrics_bam_file, csrc/dupmetrics.hip).  --optical-distance N adds the
// optical duplicates and the set-size histogram of the duplicate sets (csrc/dupsets.hip).
// `calmd` (not in the reference, which removes MD from every read it moves and leaves the rest to `samtools calmd`) is
// FileReader -> CalMD -> FileWriter: the NM and MD tags recomputed against -R on the GPU (csrc/calmd.hip; DESIGN.md
// section 28); `localrealign --calmd` puts the same module between the realigner and the writer.
//
// Deliberate differences: view -B/-E cuts QUAL to the window of SEQ; the reference cuts the
// qualities of the already shortened read a second time (algorithms/filter.cpp:188-189), which leaves fewer
// qualities than bases, bytes from behind the qualities in reads without tags, and an abort on short reads. dedup defaults to `-v --nosplit` semantics (Q1, Q3).
// --compat-nonverbose-dedup reproduces the non-verbose index bug; --split-chains K reproduces K
// split-by-chromosome chains, and --compat-split the reference's own rule for them (without
// --nosplit/--nothreads: K = min(12, threads / 2), command_dedup.cpp:46-48).  Sort by name (-b)
// gives the true name order (the reference merges name-sorted temp runs by position,
// util/read_stream_reader.h:94-97, so its output is name-sorted only within one run of -n reads).
// SAM input: every input whose first byte is '@' is SAM text (util/read_stream_reader.h:45-85), parsed into BAM
// records on the GPU (csrc/sam_parse.hip; FileReader, and stats / count / coverage); one SAM file goes into HBM as
// text and its records stay there, several inputs, a SAM file among BAM files and stdin are read on the host and
// parsed through oge_sam_parse.  `index` refuses SAM; a SAM text larger than HBM is refused, not spilled.  Where the
// reference's reader aborts or corrupts (QUAL or SEQ `*`, lowercase bases, B and H tags, integers past int32, a
// last line without its newline) the SAM specification is followed; a line that does not parse ends the command
// with its line number before anything is written.
// -F sam|fastq|bam: SAM text from view, mergesort, sort and dedup, FASTQ text from view to stdout, both
// formatted on the GPU (FileWriter::write_text).  FASTQ files (the reference's _1.fastq / _2.fastq / .fastq
// split), text output with --gpus or --index, the RAWBAM and CRAM formats and -F on localrealign fail loudly
// before anything is read.
#include <sys/resource.h>
#include <sys/time.h>

#include <cerrno>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "modules.h"

using namespace oge;

namespace {

struct Opt {
    const char *shortname, *longname;
    bool takes_value;
};

// global_options + io_options (commands.cpp:117-132) and each command's getOptions()
const Opt kGlobal[] = {{"v", "verbose", false}, {"t", "threads", true}, {"d", "nothreads", false},
                       {"T", "tmpdir", true},   {"", "nosplit", false},  {"i", "in", true},
                       {"F", "format", true},   {"c", "compression", true}, {"", "nopg", false},
                       {"", "device", true},    {"", "compat-nonverbose-dedup", false},
                       {"", "split-chains", true}, {"", "compat-split", false}, {"", "gpus", true},
                       {"", "deflate-search", true}};
const Opt kMergesort[] = {{"o", "out", true}, {"r", "region", true},  {"q", "mapq", true},
                          {"b", "byname", false}, {"n", "n", true}, {"C", "compresstempfiles", false},
                          {"M", "markduplicates", false}, {"R", "removeduplicates", false}, {"", "index", false},
                          {"L", "regions", true}, {"", "noindex", false}, {"", "metrics", true},
                          {"", "optical-distance", true}};
const Opt kDedup[] = {{"o", "out", true}, {"r", "remove", false}, {"", "index", false}, {"", "metrics", true},
                      {"", "optical-distance", true}};
const Opt kDupmetrics[] = {{"o", "out", true}, {"", "optical-distance", true}};
const Opt kView[] = {{"o", "out", true}, {"n", "count", true}, {"q", "mapq", true}, {"l", "length", true},
                     {"B", "trimbegin", true}, {"E", "trimend", true}, {"r", "region", true}, {"L", "regions", true},
                     {"", "noindex", false}};
const Opt kIndex[] = {{"o", "out", true}};
const Opt kStats[] = {{"I", "inserts", false}, {"L", "lengths", false}};
const Opt kCoverage[] = {{"o", "out", true}, {"b", "binsize", true}, {"", "omituncoveredbases", false},
                         {"V", "verifymapping", false}, {"S", "strict", false}};
const Opt kCompare[] = {{"r", "region", true}, {"p", "print", false}};
const Opt kTargets[] = {{"o", "out", true}, {"", "maxinterval", true}, {"", "gap", true}};
const Opt kRealign[] = {{"o", "out", true}, {"R", "reference", true}, {"L", "intervals", true}, {"", "auto-targets", false},
                        {"", "calmd", false}};
const Opt kCalmd[] = {{"o", "out", true}, {"R", "reference", true}, {"", "index", false}};

struct Parsed {
    std::map<std::string, std::vector<std::string>> vm;  // long name -> values ("" for flags)
    std::vector<std::string> inputs;
    bool count(const char *k) const { return vm.count(k) != 0; }
    std::string get(const char *k, const std::string &def) const {
        auto it = vm.find(k);
        return it == vm.end() || it->second.empty() ? def : it->second.back();
    }
};

bool parse(int argc, const char **argv, const std::vector<Opt> &opts, Parsed &p) {
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        const Opt *o = nullptr;
        std::string val;
        bool have_val = false;
        if (a.size() > 2 && a[0] == '-' && a[1] == '-') {
            std::string k = a.substr(2);
            size_t eq = k.find('=');
            if (eq != std::string::npos) {
                val = k.substr(eq + 1);
                k = k.substr(0, eq);
                have_val = true;
            }
            for (auto &x : opts)
                if (k == x.longname) o = &x;
        } else if (a.size() >= 2 && a[0] == '-' && a != "-") {
            std::string k = a.substr(1, 1);
            for (auto &x : opts)
                if (k == x.shortname) o = &x;
            if (o && a.size() > 2) {
                val = a.substr(2);
                have_val = true;
            }
        } else {
            p.inputs.push_back(a);
            continue;
        }
        if (!o) {
            fprintf(stderr, "Error: unrecognised option '%s'\n", a.c_str());
            return false;
        }
        if (o->takes_value && !have_val) {
            if (i + 1 >= argc) {
                fprintf(stderr, "Error: the required argument for option '--%s' is missing\n", o->longname);
                return false;
            }
            val = argv[++i];
        }
        p.vm[o->longname].push_back(o->takes_value ? val : "");
    }
    for (auto &v : p.vm["in"]) p.inputs.push_back(v);
    p.vm.erase("in");
    return true;
}

void usage_top() {
    fprintf(stderr, "Usage:\n    openge command [options]\n\nCommands: mergesort (alias: sort), dedup, localrealign, view, index, stats, count, coverage,\n"
                    "          compare, targets, dupmetrics, calmd, version\n"
                    "\n    Inputs are BAM files or SAM text (first byte '@'; also on stdin, and mixed with BAM files); SAM is parsed\n"
                    "    on the GPU.  index takes BAM only.\n"
                    "\n    openge view [-o out] [-n N] [-q MAPQ] [-l LEN] [-r REGION] [-L FILE] [-B N] [-E N] in.bam|in.sam\n"
                    "                                        the reads that pass the filters (-l: 64, 64-72, -64 or +64), as SAM\n"
                    "                                        on stdout, else in the format of -F or of the output name's suffix;\n"
                    "                                        -B / -E trim bases from the read ends, FASTQ only\n"
                    "    view / mergesort / sort -L FILE     keep the reads of at least one region of FILE (one per line in the\n"
                    "                                        syntax of -r; blank lines and lines starting with # are skipped),\n"
                    "                                        each read once, in input order; with -r: of either\n"
                    "    view / mergesort / sort -r / -L     with in.bam.bai (or in.bai) beside one BAM input, not older than it,\n"
                    "                                        only the blocks the index names are read; --noindex: always the\n"
                    "                                        whole file.  The output is the same either way.\n"
                    "    -F sam | fastq | bam                output format of view, mergesort, sort and dedup (SAM and FASTQ text are\n"
                    "                                        formatted on the GPU; FASTQ only from view to stdout; not with --gpus\n"
                    "                                        or --index)\n"
                    "    openge index in.bam [-o out.bai]    BAM index of a coordinate-sorted file (default in.bam.bai)\n"
                    "    mergesort / sort / dedup --index    also write <out>.bai (one GPU, file output, coordinate order)\n"
                    "    openge stats [-I] [-L] in.bam|in.sam  flag counts, Sorted: Yes/No, insert sizes (-I), read lengths (-L)\n"
                    "    openge count in.bam|in.sam          the number of reads\n"
                    "    openge coverage [-o out.tsv] [-b N] [--omituncoveredbases] in.bam|in.sam\n"
                    "                                        depth per bin of N bases (default 100); one file, one GPU\n"
                    "    openge compare [-r REGION]... [-p] ref.bam|ref.sam other.bam|other.sam [more...]\n"
                    "                                        read placements (contig, position, CIGAR) of every later file that\n"
                    "                                        the first one lacks (added) or has more of (removed), per region\n"
                    "                                        (reads that START in it); -p prints each one; one GPU, no stdin\n"
                    "    openge targets [-o out.intervals] [--maxinterval N] [--gap N] in.bam|in.sam\n"
                    "                                        realignment target intervals (contig:start-stop) from the reads' own\n"
                    "                                        indels, computed on the GPU: events closer than --gap (default 0) merge,\n"
                    "                                        intervals of --maxinterval (default 500) bases or more are dropped;\n"
                    "                                        the file localrealign -L takes; one file, one GPU, no stdin\n"
                    "    openge localrealign -R ref.fa (-L targets.intervals | --auto-targets) [-T tmpdir] [-o out.bam] in.bam\n"
                    "                                        --auto-targets: the intervals of `openge targets` at its defaults,\n"
                    "                                        computed from the input's records (kept in a file in tmpdir meanwhile)\n"
                    "    openge calmd -R ref.fa [-o out] [-F sam] [-c level] [--index] in.bam|in.sam\n"
                    "                                        the NM and MD tags of every mapped read recomputed against ref.fa on\n"
                    "                                        the GPU, as samtools calmd without options: a tag that is right\n"
                    "                                        stays, any other is replaced at the record's end; BAM (default) or\n"
                    "                                        SAM out; one GPU, the input resident in HBM\n"
                    "    openge localrealign ... --calmd     the same step between the realigner and the writer, with its -R\n"
                    "    openge dedup --metrics FILE / mergesort|sort -M --metrics FILE\n"
                    "                                        also write Picard's duplication metrics of the marked records to\n"
                    "                                        FILE: per library the reads and pairs examined, the duplicates,\n"
                    "                                        PERCENT_DUPLICATION, ESTIMATED_LIBRARY_SIZE, and the ROI histogram\n"
                    "                                        when there is one library; counted on the GPU before -r / -R removes\n"
                    "                                        anything; FILE is neither the output nor stdout\n"
                    "    openge dupmetrics [-o out.txt] in.bam|in.sam\n"
                    "                                        the same metrics of a file that is already marked, by this tool or\n"
                    "                                        another (default: stdout); one file, one GPU, no stdin\n"
                    "    --optical-distance N                with dedup --metrics, mergesort|sort -M|-R --metrics and dupmetrics:\n"
                    "                                        the duplicate sets of the records, computed on the GPU: fills\n"
                    "                                        READ_PAIR_OPTICAL_DUPLICATES (pairs of one set, read group and tile\n"
                    "                                        within N pixels in x and y of one another, by the tile:x:y at the end\n"
                    "                                        of 5- or 7-field read names; 100, or 2500 on patterned flow cells),\n"
                    "                                        takes them out of ESTIMATED_LIBRARY_SIZE, and writes the set-size\n"
                    "                                        histogram; one GPU, the records resident in HBM\n"
                    "\nGPU options (every command):\n"
                    "    --device N              first GPU\n"
                    "    --gpus G                ranks over G GPUs\n"
                    "    --deflate-search NAME   match search of the GPU BAM writer: fast (default), near, span or\n"
                    "                            near+span (smaller files; see oge_ctx_set_deflate_search)\n");
}

}  // namespace

int main(int argc, const char **argv) {
    if (argc == 1) {
        usage_top();
        return 0;
    }
    std::string cmd = argv[1];
    if (cmd == "sort") cmd = "mergesort";  // the reference has no `sort` command
    if (cmd == "version") {
        printf("openge 0.3-dev (openge_amd MI355X path: %s)\n", oge_version());
        return 0;
    }
    if (cmd == "help") {
        usage_top();
        return 0;
    }
    std::vector<Opt> opts(std::begin(kGlobal), std::end(kGlobal));
    if (cmd == "mergesort") opts.insert(opts.end(), std::begin(kMergesort), std::end(kMergesort));
    else if (cmd == "dedup") opts.insert(opts.end(), std::begin(kDedup), std::end(kDedup));
    else if (cmd == "localrealign") opts.insert(opts.end(), std::begin(kRealign), std::end(kRealign));
    else if (cmd == "view") opts.insert(opts.end(), std::begin(kView), std::end(kView));
    else if (cmd == "index") opts.insert(opts.end(), std::begin(kIndex), std::end(kIndex));
    else if (cmd == "stats") opts.insert(opts.end(), std::begin(kStats), std::end(kStats));
    else if (cmd == "count") ;  // no options of its own (commands/command_count.cpp)
    else if (cmd == "coverage") opts.insert(opts.end(), std::begin(kCoverage), std::end(kCoverage));
    else if (cmd == "compare") opts.insert(opts.end(), std::begin(kCompare), std::end(kCompare));
    else if (cmd == "targets") opts.insert(opts.end(), std::begin(kTargets), std::end(kTargets));
    else if (cmd == "dupmetrics") opts.insert(opts.end(), std::begin(kDupmetrics), std::end(kDupmetrics));
    else if (cmd == "calmd") opts.insert(opts.end(), std::begin(kCalmd), std::end(kCalmd));
    else {
        fprintf(stderr, "Unknown command %s.\n", argv[1]);
        return -1;
    }
    // command_line (commands.cpp:36-40): "openge " + every argument after `openge`, space-terminated
    std::string command_line = "openge ";
    for (int i = 1; i < argc; ++i) {
        command_line += argv[i];
        command_line += " ";
    }
    Parsed p;
    if (!parse(argc - 1, argv + 1, opts, p)) return -1;
    if (p.inputs.empty()) p.inputs.push_back("stdin");

    ChainContext cc;
    cc.verbose = p.count("verbose");
    cc.threads = atoi(p.get("threads", std::to_string(std::max(1u, std::thread::hardware_concurrency()))).c_str());
    cc.device = atoi(p.get("device", "0").c_str());
    cc.gpus = std::max(1, atoi(p.get("gpus", "1").c_str()));  // ranks over RCCL / xGMI
    AlgorithmModule::setVerbose(cc.verbose);
    const int level = atoi(p.get("compression", "6").c_str());
    const bool compat = p.count("compat-nonverbose-dedup");
    int split = atoi(p.get("split-chains", "0").c_str());
    if (p.count("compat-split") && !p.count("nosplit") && !p.count("nothreads")) split = std::min(12, cc.threads / 2);
    if (split > 1 && compat) {
        fprintf(stderr, "openge: split chains with --compat-nonverbose-dedup are not supported\n");
        return -1;
    }
    if (p.count("deflate-search")) {
        // through the environment: every context the command creates (the chain's, each rank's) reads it
        const std::string s = p.get("deflate-search", "fast");
        if (s != "fast" && s != "near" && s != "span" && s != "near+span") {
            fprintf(stderr, "openge: --deflate-search %s: fast, near, span or near+span\n", s.c_str());
            return -1;
        }
        setenv("OGE_DEFLATE_SEARCH", s.c_str(), 1);
    }
    // the output format (file_writer.cpp:45-67, command_view.cpp:64-95): -F, then for view the output name's suffix,
    // then SAM when view writes to stdout, else BAM; what is not provided fails before anything is read
    const std::string out_name = p.get("out", "stdout");
    const bool out_stdout = out_name == "stdout" || out_name == "-";
    FileFormat fmt = FORMAT_BAM;
    const bool chain_cmd = cmd == "view" || cmd == "mergesort" || cmd == "dedup" || cmd == "localrealign" || cmd == "calmd";
    if (chain_cmd) {
        if (p.count("format")) {
            FileWriter probe;
            if (probe.setFormat(p.get("format", "bam"))) return -1;
            fmt = probe.getFileFormat();
        } else if (cmd == "view") {
            fmt = detect_file_format(out_name);
            if (fmt == FORMAT_UNKNOWN) fmt = FORMAT_BAM;
        }
        if (cmd == "view" && (p.count("trimbegin") || p.count("trimend")) && fmt != FORMAT_FASTQ) {  // command_view.cpp:89-92
            fprintf(stderr, "Trimming reads is only supported for the FASTQ format at this time. Aborting.\n");
            return -1;
        }
        if (cmd == "view" && !p.count("format") && detect_file_format(out_name) == FORMAT_UNKNOWN && out_stdout) fmt = FORMAT_SAM;
        if (fmt == FORMAT_RAWBAM || fmt == FORMAT_CRAM) {  // file_writer.cpp:192-195
            fprintf(stderr, "Unsupported output file format selected. Aborting.\n");
            return -1;
        }
        const bool text = fmt == FORMAT_SAM || fmt == FORMAT_FASTQ;
        const char *why = !text                                  ? nullptr
                          : cmd == "localrealign"                ? "localrealign (BAM only)"
                          : cc.gpus > 1                          ? "--gpus"
                          : p.count("index")                     ? "--index"
                          : fmt == FORMAT_FASTQ && cmd != "view" ? "this command (only view writes FASTQ)"
                          : fmt == FORMAT_FASTQ && !out_stdout   ? "an output file (only -o stdout: the _1.fastq / _2.fastq / .fastq split is not provided)"
                                                                 : nullptr;
        if (why) {
            fprintf(stderr, "openge: %s output is not provided with %s\n", fmt == FORMAT_SAM ? "SAM" : "FASTQ", why);
            return -1;
        }
        if (cmd == "view" && cc.gpus > 1) {
            fprintf(stderr, "openge view: --gpus is not provided\n");
            return -1;
        }
        if (cmd == "view" && (atoi(p.get("trimbegin", "0").c_str()) < 0 || atoi(p.get("trimend", "0").c_str()) < 0)) {
            fprintf(stderr, "openge view: -B / -E must not be negative\n");
            return -1;
        }
    }
    if (p.count("index")) {  // what the index is not provided with fails before anything is read or written
        const char *why = p.get("out", "stdout") == "stdout" || p.get("out", "stdout") == "-" ? "output to stdout"
                          : cc.gpus > 1                                                        ? "--gpus"
                          : p.count("byname")                                                  ? "-b (sort by name)"
                                                                                               : nullptr;
        if (why) {
            fprintf(stderr, "openge: --index is not provided with %s\n", why);
            return -1;
        }
    }
    if (cmd == "index" && (p.inputs.size() != 1 || p.inputs[0] == "stdin" || p.inputs[0] == "-")) {
        fprintf(stderr, "openge index: one BAM file is required\n");
        return -1;
    }
    const bool qc = cmd == "stats" || cmd == "count" || cmd == "coverage";
    if (qc) {  // refused before anything is read
        const char *c = cmd.c_str();
        if (p.inputs.size() != 1 || p.inputs[0] == "stdin" || p.inputs[0] == "-") {
            fprintf(stderr, "openge %s: one BAM file is required\n", c);
            return -1;
        }
        if (cc.gpus > 1) {
            fprintf(stderr, "openge %s: --gpus is not provided\n", c);
            return -1;
        }
        if (p.count("verifymapping") || p.count("strict")) {
            fprintf(stderr, "openge coverage: -V/--verifymapping and -S/--strict are not provided\n");
            return -1;
        }
        if (cmd == "coverage" && atoi(p.get("binsize", "100").c_str()) < 1) {
            fprintf(stderr, "openge coverage: --binsize must be at least 1\n");
            return -1;
        }
    }
    if (cmd == "compare") {  // refused before anything is read
        for (auto &in : p.inputs)
            if (in == "stdin" || in == "-") {
                fprintf(stderr, "openge compare: stdin is not provided as an input (every file is read on its own, the first one for every other)\n");
                return -1;
            }
        if (cc.gpus > 1) {
            fprintf(stderr, "openge compare: --gpus is not provided\n");
            return -1;
        }
    }
    if (cmd == "targets") {  // refused before anything is read
        if (p.inputs.size() != 1 || p.inputs[0] == "stdin" || p.inputs[0] == "-") {
            fprintf(stderr, "openge targets: one BAM or SAM file is required (stdin is not provided)\n");
            return -1;
        }
        if (cc.gpus > 1) {
            fprintf(stderr, "openge targets: --gpus is not provided\n");
            return -1;
        }
        if (atoi(p.get("maxinterval", "500").c_str()) < 1) {
            fprintf(stderr, "openge targets: --maxinterval must be at least 1\n");
            return -1;
        }
        if (atoi(p.get("gap", "0").c_str()) < 0) {
            fprintf(stderr, "openge targets: --gap must not be negative\n");
            return -1;
        }
    }
    if (cmd == "dupmetrics") {  // refused before anything is read
        if (p.inputs.size() != 1 || p.inputs[0] == "stdin" || p.inputs[0] == "-") {
            fprintf(stderr, "openge dupmetrics: one BAM or SAM file is required (stdin is not provided)\n");
            return -1;
        }
        if (cc.gpus > 1) {
            fprintf(stderr, "openge dupmetrics: --gpus is not provided\n");
            return -1;
        }
    }
    if (p.count("metrics")) {  // refused before anything is read
        const std::string mf = p.get("metrics", "");
        if (cmd == "mergesort" && !p.count("markduplicates") && !p.count("removeduplicates")) {
            fprintf(stderr, "openge mergesort: --metrics needs -M or -R (there is nothing to count without the duplicate marking)\n");
            return -1;
        }
        if (mf.empty() || mf == "stdout" || mf == "-") {
            fprintf(stderr, "openge %s: --metrics needs a file name (stdout is not provided)\n", cmd.c_str());
            return -1;
        }
        if (mf == out_name) {
            fprintf(stderr, "openge %s: --metrics names the output file\n", cmd.c_str());
            return -1;
        }
    }
    int64_t optical_distance = -1;
    if (p.count("optical-distance")) {  // refused before anything is read
        const std::string v = p.get("optical-distance", "");
        char *end = nullptr;
        errno = 0;
        const long long d = strtoll(v.c_str(), &end, 10);
        if (v.empty() || v[0] < '0' || v[0] > '9' || *end || errno || d > INT32_MAX) {
            fprintf(stderr, "openge %s: --optical-distance needs a number from 0 to 2147483647\n", cmd.c_str());
            return -1;
        }
        if (cmd != "dupmetrics" && !p.count("metrics")) {
            fprintf(stderr, "openge %s: --optical-distance needs --metrics (the optical duplicates go into the metrics file)\n", cmd.c_str());
            return -1;
        }
        if (cc.gpus > 1) {
            fprintf(stderr, "openge %s: --optical-distance is not provided with --gpus\n", cmd.c_str());
            return -1;
        }
        if (split > 1 || compat) {
            fprintf(stderr, "openge %s: --optical-distance is not provided with split chains or --compat-nonverbose-dedup\n", cmd.c_str());
            return -1;
        }
        optical_distance = d;
    }
    const bool calmd = cmd == "calmd" || (cmd == "localrealign" && p.count("calmd"));
    if (calmd) {  // refused before anything is read
        if (cmd == "calmd" && (!p.count("reference") || p.vm["reference"].size() != 1)) {
            fprintf(stderr, "openge calmd: one FASTA reference file is required (-R ref.fa)\n");
            return -1;
        }
        if (cc.gpus > 1) {
            fprintf(stderr, "openge %s: %s is not provided with --gpus\n", cmd.c_str(), cmd == "calmd" ? "calmd" : "--calmd");
            return -1;
        }
    }
    if (cmd == "localrealign" && p.count("auto-targets") && p.count("intervals")) {
        fprintf(stderr, "openge localrealign: -L and --auto-targets exclude each other\n");
        return -1;
    }
    if (p.count("regions")) {  // an unreadable -L file is refused before anything is read
        const std::string rf = p.get("regions", "");
        FILE *f = fopen(rf.c_str(), "r");
        if (!f) {
            fprintf(stderr, "openge: cannot read the regions file %s\n", rf.c_str());
            return -1;
        }
        fclose(f);
    }
    timeval t0;
    gettimeofday(&t0, nullptr);
    // one input file on one GPU: its bytes come off the disk / page cache while HIP initialises -- unless the
    // reader will take only the blocks an index names (regions, an index beside the file, no --noindex)
    std::string bai_path, bai_why;
    const bool indexed = (cmd == "view" || cmd == "mergesort") && (p.count("region") || p.count("regions")) && !p.count("noindex") &&
                         p.inputs.size() == 1 && cc.gpus == 1 && FileReader::index_beside(p.inputs[0], bai_path, bai_why);
    if (p.inputs.size() == 1 && p.inputs[0] != "stdin" && cc.gpus == 1 && !indexed) prefetch_input(p.inputs[0]);
    if (oge_ctx_create(cc.device, &cc.ctx)) {
        fprintf(stderr, "openge: %s\n", oge_last_error(nullptr));
        return -1;
    }
    const char *pool = getenv("OGE_POOL");  // default on: the chain's modules share one memory pool
    if (!(pool && std::string(pool) == "0") && oge_ctx_set_pool(cc.ctx, 1)) {
        fprintf(stderr, "openge: %s\n", oge_last_error(cc.ctx));
        return -1;
    }
    if (calmd && !CalMD::fitsDevice(cc, p.inputs, p.get("reference", ""))) {  // refused before anything is read
        oge_ctx_destroy(cc.ctx);
        return -1;
    }
    if (cmd == "index") {
        const int r = index_bam_file(cc, p.inputs[0], p.get("out", p.inputs[0] + ".bai"));
        oge_ctx_destroy(cc.ctx);
        return r;
    }
    if (cmd == "compare") {
        const int r = compare_files(cc, p.inputs, p.count("region") ? p.vm["region"] : std::vector<std::string>(), p.count("print"));
        oge_ctx_destroy(cc.ctx);
        return r;
    }
    if (cmd == "targets") {
        const int r = targets_bam_file(cc, p.inputs[0], p.get("out", "stdout"), atoi(p.get("maxinterval", "500").c_str()),
                                       atoi(p.get("gap", "0").c_str()));
        oge_ctx_destroy(cc.ctx);
        return r;
    }
    if (cmd == "dupmetrics") {
        const int r = dupmetrics_bam_file(cc, p.inputs[0], p.get("out", "stdout"), command_line, optical_distance);
        oge_ctx_destroy(cc.ctx);
        return r;
    }
    if (qc) {
        const int r = cmd == "stats"   ? stats_bam_file(cc, p.inputs[0], p.count("inserts"), p.count("lengths"))
                      : cmd == "count" ? count_bam_file(cc, p.inputs[0])
                                       : coverage_bam_file(cc, p.inputs[0], p.get("out", "stdout"), atoi(p.get("binsize", "100").c_str()),
                                                           p.count("omituncoveredbases"));
        oge_ctx_destroy(cc.ctx);
        return r;
    }

    FileReader reader;
    FileWriter writer;
    reader.addFiles(p.inputs);
    reader.setNoIndex(p.count("noindex"));
    writer.setFilename(p.get("out", "stdout"));
    writer.setIndex(p.count("index"));
    if (!p.count("nopg")) writer.addProgramLine(command_line);
    writer.setCompressionLevel(level);
    if (p.count("format") && writer.setFormat(p.get("format", "bam"))) return -1;

    int ret = 0;
    if (cmd == "view") {  // command_view.cpp:44-100
        Filter filter;
        if (p.count("count")) filter.setCountLimit((int)std::min<long long>(INT32_MAX, atoll(p.get("count", "0").c_str())));
        if (p.count("mapq")) filter.setQualityLimit(atoi(p.get("mapq", "0").c_str()));
        if (p.count("length")) filter.setReadLengths(p.get("length", ""));
        if (p.count("trimbegin")) filter.setTrimBeginLength(atoi(p.get("trimbegin", "0").c_str()));
        if (p.count("trimend")) filter.setTrimEndLength(atoi(p.get("trimend", "0").c_str()));
        if (p.count("region")) filter.setRegion(p.get("region", ""));
        if (p.count("regions") && !filter.setRegionsFile(p.get("regions", ""))) return -1;
        writer.setTrim(atoi(p.get("trimbegin", "0").c_str()), atoi(p.get("trimend", "0").c_str()));
        writer.setDefaultFormat(out_stdout ? FORMAT_SAM : FORMAT_BAM);
        reader.addSink(&filter);
        filter.addSink(&writer);
        ret = writer.runChain(cc);
    } else if (cmd == "mergesort") {
        bool dedup = p.count("markduplicates") || p.count("removeduplicates");
        Filter filter;
        ReadSorter sorter;
        MarkDuplicates md;
        sorter.setSortBy(p.count("byname") ? BamHeaderModel::QUERYNAME : BamHeaderModel::COORDINATE);
        sorter.setCompressTempFiles(p.count("compresstempfiles"));
        sorter.setAlignmentsPerTempfile(atoi(p.get("n", "500000").c_str()));
        if (p.count("region") || p.count("mapq") || p.count("regions")) {  // command_mergesort.cpp:82-92
            if (p.count("region")) filter.setRegion(p.get("region", ""));
            if (p.count("regions") && !filter.setRegionsFile(p.get("regions", ""))) return -1;
            if (p.count("mapq")) filter.setQualityLimit(atoi(p.get("mapq", "0").c_str()));
            reader.addSink(&filter);
            filter.addSink(&sorter);
        } else {
            reader.addSink(&sorter);
        }
        if (dedup) {
            md.removeDuplicates = p.count("removeduplicates");
            md.compatNonverbose = compat;
            md.splitChains = split;
            md.metricsFilename = p.get("metrics", "");
            md.metricsCommandLine = command_line;
            md.opticalDistance = optical_distance;
            sorter.addSink(&md);
            md.addSink(&writer);
        } else {
            sorter.addSink(&writer);
        }
        ret = writer.runChain(cc);
        if (cc.verbose && dedup) fprintf(stderr, "Marked %llu records as duplicates.\n", (unsigned long long)md.duplicates);
    } else if (cmd == "calmd") {
        CalMD cm;
        cm.setReferenceFilename(p.get("reference", ""));
        reader.addSink(&cm);
        cm.addSink(&writer);
        ret = writer.runChain(cc);
    } else if (cmd == "dedup") {
        MarkDuplicates md;
        md.removeDuplicates = p.count("remove");
        md.compatNonverbose = compat;
        md.splitChains = split;
        md.metricsFilename = p.get("metrics", "");
        md.metricsCommandLine = command_line;
        md.opticalDistance = optical_distance;
        reader.addSink(&md);
        md.addSink(&writer);
        ret = writer.runChain(cc);
        if (cc.verbose) fprintf(stderr, "Marked %llu records as duplicates.\n", (unsigned long long)md.duplicates);
    } else {
        if (!p.count("reference") || p.vm["reference"].size() != 1) {
            fprintf(stderr, "One FASTA reference file is required.\n");
            return -1;
        }
        const bool auto_targets = p.count("auto-targets");
        if (!auto_targets && (!p.count("intervals") || p.vm["intervals"].size() != 1)) {
            fprintf(stderr, "One intervals file is required.\n");
            return -1;
        }
        LocalRealignment lr;
        lr.verbose = cc.verbose;
        lr.setReferenceFilename(p.get("reference", ""));
        lr.setIntervalsFilename(p.get("intervals", ""));
        lr.setAutoTargets(auto_targets, p.get("tmpdir", "/tmp"));
        CalMD cm;
        cm.setReferenceFilename(p.get("reference", ""));
        reader.addSink(&lr);
        if (calmd) {
            lr.addSink(&cm);
            cm.addSink(&writer);
        } else {
            lr.addSink(&writer);
        }
        ret = writer.runChain(cc);
    }
    cc.close_ranks();
    oge_ctx_destroy(cc.ctx);
    if (cc.verbose) {  // commands.cpp:91-108
        rusage r;
        getrusage(RUSAGE_SELF, &r);
        timeval t1;
        gettimeofday(&t1, nullptr);
        double el = (t1.tv_sec - t0.tv_sec) + 1e-6 * (t1.tv_usec - t0.tv_usec);
        fprintf(stderr, "Elapsed time: %3ldm%06.3fs\n", (long)el / 60, el - 60 * ((long)el / 60));
        fprintf(stderr, "Max mem: %6ld MB\n", r.ru_maxrss / 1024);
    }
    return ret;
}
