// modules.h -- the AlgorithmModule operator API of OpenGE (algorithms/algorithm_module.h:33-107),
// re-designed for MI355X: a chain of modules hands ONE batch of records (the whole input) from
// module to module instead of streaming OGERead* through polled per-module queues.  Records stay in
// HBM between device modules (ReadSorter -> MarkDuplicates is fused into one device pipeline), and
// only the file endpoints touch host memory.  Module names, setters and defaults follow the
// reference; each class cites the module it replaces.
//
// Built on the C ABI only (include/openge_hip.h): this layer is what an OpenGE maintainer would
// link against, and it contains no HIP code of its own.
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../../include/openge_hip.h"
#include "bam_layout.h"
#include "bamio.h"
#include "file_load.h"

namespace oge {

// the struct by a name of its own: the plain name is the host-buffer entry point's
using OgeDupMetrics = struct ::oge_dup_metrics;
using OgeDupSetsLib = struct ::oge_dup_sets_lib;

struct ChainContext;

// Records of one chain, resident in host memory, HBM, or both.
struct ReadBatch {
    BamHeaderModel header;
    std::vector<std::string> ref_names;
    uint64_t n = 0;
    // host form
    bytevec recs;                     // + 16 bytes of slack
    std::vector<uint64_t> offs;       // n + 1
    bool host_valid = false;
    // device form
    uint8_t *d_recs = nullptr;
    uint64_t *d_offs = nullptr;
    uint64_t d_bytes = 0;
    bool dev_valid = false;
    // dedup output applied by the writer (-r / -R: records carrying 0x400 are not written)
    bool drop_duplicates = false;
    // multi-GPU (--gpus G): the records as G slices in rank order, each in its rank's HBM (owned by
    // the rank's context); when set, the host and device forms above are unused
    struct Slice {
        oge_ctx *ctx;
        uint8_t *d_recs;
        uint64_t *d_offs;  // n + 1 byte offsets from d_recs
        uint64_t n;
    };
    std::vector<Slice> slices;
    // multi-GPU input (--gpus G, one BAM file): the records as G input shards in rank order (contiguous
    // ranges of the file's records, each decoded by its rank from its own byte range of the file,
    // oge_bgzf_decode_shard), owned by the ranks' contexts; run_ranks takes them as they are
    std::vector<Slice> shards;
    // inputs larger than HBM: the output is produced range by range when the writer asks for it
    // (oge_sort_markdup_chunked); each range is handed to `sink` in output order
    using RangeSink = std::function<int(const uint8_t *d_recs, const uint64_t *d_offs, uint64_t n)>;
    std::function<int(ChainContext &, const RangeSink &)> produce;

    uint64_t bytes() const { return host_valid ? offs[n] : d_bytes; }
};

struct ChainContext {
    oge_ctx *ctx = nullptr;
    int device = 0;
    int threads = 0;
    bool verbose = false;
    // --gpus G: rank contexts (rank 0 = ctx, rank g on device (device + g) % devices; ranks share a
    // device when there are fewer devices than ranks) and their communicators
    int gpus = 1;
    std::vector<oge_ctx *> rank_ctx;
    std::vector<oge_comm *> comms;
    int init_ranks();
    void close_ranks();
    int fail(const std::string &where);  // prints oge_last_error, returns -1
    int to_device(ReadBatch &b);
    int to_host(ReadBatch &b);
    void free_device(ReadBatch &b);
};

class AlgorithmModule {
public:
    virtual ~AlgorithmModule() {}
    void addSink(AlgorithmModule *sink) { sink_ = sink; sink->source_ = this; }
    // AlgorithmModule::runChain (algorithm_module.cpp:92-116): run every module of the chain that
    // ends at this one, from its first source.  Returns 0 or the first failing module's status
    // (the reference always returns 0).
    int runChain(ChainContext &cc);
    static void setVerbose(bool v) { verbose_ = v; }
    static bool isVerbose() { return verbose_; }
    const char *name() const { return name_; }
    AlgorithmModule *sink() const { return sink_; }

protected:
    explicit AlgorithmModule(const char *name) : name_(name) {}
    // consume `b` (the previous module's output) in place; sources ignore it and fill it
    virtual int runInternal(ChainContext &cc, ReadBatch &b) = 0;
    AlgorithmModule *source_ = nullptr, *sink_ = nullptr;
    static bool verbose_;
    const char *name_;
    friend class ReadSorter;
};

// FileReader (algorithms/file_reader.cpp:29-63): BAM and SAM input(s); an input whose first byte is '@' is SAM
// text (util/read_stream_reader.h:45-85) and is parsed into records on the GPU: one SAM file as text in HBM
// (oge_sam_lines_dev / _size_dev / _emit_dev, the records stay there), several inputs, a SAM file among BAM
// files and stdin through oge_sam_parse on the host path.  Several inputs are interleaved as
// the reference's MultiReader does (a ByPosition merge of the file heads,
// util/read_stream_reader.h:132-153) unless a ReadSorter follows, which makes the interleaving
// irrelevant; the header is the first file's (a differing dictionary only warns, :116-124).
// The index is asked for [left_pos - kIndexWiden, right_pos]: the Filter keeps a record when pos + l_seq >=
// left_pos, and l_seq is below the record walk's block_size cap (OGE_MAX_BLOCK_SIZE, the constant inflate.hip's
// walk tests), the largest record the device reader admits; the index itself was built from reference spans,
// which can be shorter (soft clips, insertions).  A record beyond the cap inside the decoded ranges fails the
// walk and gives the full scan; one outside them that reaches a region with more than the cap of clipped or
// inserted bases is not found through the index (the host reader, which the full scan of such a file falls to,
// keeps it).
constexpr int32_t kIndexWiden = OGE_MAX_BLOCK_SIZE;

class FileReader : public AlgorithmModule {
public:
    FileReader() : AlgorithmModule("FileReader") {}
    void addFile(const std::string &f) { files_.push_back(f); }
    void addFiles(const std::vector<std::string> &f) { files_.insert(files_.end(), f.begin(), f.end()); }
    void setLoadStringData(bool) {}  // the record arena always keeps the full record bytes
    void setNoIndex(bool on) { no_index_ = on; }  // --noindex: never read a .bai
    // <path>.bai, or <path minus ".bam">.bai, when it exists and is not older than the file; else `why` says
    // what is missing
    static bool index_beside(const std::string &path, std::string &bai, std::string &why);
    // outside a chain (compare_files): this reader's files into b, the records resident in HBM
    int load(ChainContext &cc, ReadBatch &b) {
        const int rc = runInternal(cc, b);
        return rc ? rc : cc.to_device(b);
    }
protected:
    int runInternal(ChainContext &cc, ReadBatch &b) override;
    // One BGZF file straight into HBM: inflate + record walk on the GPU (returns 1 when the host
    // reader should take over, e.g. to report a format error with the reference's message).
    int read_device(ChainContext &cc, ReadBatch &b, const std::string &path);
    // --gpus G: every rank reads and decodes its own byte range of the one input file (b.shards)
    int read_sharded(ChainContext &cc, ReadBatch &b, const std::string &path);
    // FileReader -> Filter with regions, one BAM file, one GPU, an index beside the file: only the blocks the
    // index names for the regions (widened by kIndexWiden) are read, inflated and walked (oge_bai_open,
    // oge_bai_query_dev, oge_bam_decode_ranges_dev); the Filter then runs over those records as over all of
    // them.  0 = done, 1 = the full scan takes over (one [openge] line under -v says why), -1 = a region does
    // not parse (reported).
    int read_indexed(ChainContext &cc, ReadBatch &b, const std::string &path);
    bool no_index_ = false;
    bool sink_takes_shards() const;
    bool sink_sorts() const;
    static int merge_inputs(ReadBatch &b, const std::vector<uint64_t> &file_end, int threads);
    std::vector<std::string> files_;
};

// Filter (algorithms/filter.h:30-70, filter.cpp:185-249): mergesort's -r region / -q mapq, as a
// device compaction (oge_filter_records_dev).  Trimming (setTrimBeginLength/EndLength, `view -B/-E`)
// drops the reads it would leave empty (len > trim total); the cut itself is made where the FASTQ text
// is formatted (FileWriter::setTrim), the only format the reference allows it with.
// addRegion / setRegionsFile (view / mergesort -L): any number of regions in setRegion's syntax; a record passes
// when at least one of them holds, and is written once (oge_filter_regions_dev when there is more than one).
class Filter : public AlgorithmModule {
public:
    Filter() : AlgorithmModule("Filter") { oge_filter_opts_init(&opts_); }
    void setRegion(const std::string &region) { region_ = region; has_region_ = true; }
    std::string getRegion() const { return region_; }
    void addRegion(const std::string &region) { more_regions_.push_back({region, 0}); }
    // one region per line, blank lines and lines starting with '#' skipped; false (with a message) when the
    // file cannot be read.  The lines are parsed against the header's dictionary: by the FileReader from a look
    // at the first input's header, so a line that does not parse ends the chain with its line number before any
    // input is read, and again when the module runs (a pipe's header is known only then).
    bool setRegionsFile(const std::string &path);
    bool hasRegions() const { return has_region_ || !more_regions_.empty(); }
    // every region (-r first, then the list) against the header's dictionary; -1 with the messages printed
    int parseRegions(const BamHeaderModel &h, std::vector<oge_region> &out) const;
    void setCountLimit(int ct) { opts_.count_limit = ct < 0 ? 0 : (uint64_t)ct; }
    size_t getCountLimit() const { return opts_.count_limit; }
    void setQualityLimit(int mapq) { opts_.mapq_min = mapq; }
    int getQualityLimit() const { return opts_.mapq_min; }
    void setMinimumReadLength(int l) { opts_.min_len = l; }
    void setMaximumReadLength(int l) { opts_.max_len = l; }
    void setTrimBeginLength(int l) { trim_begin_ = l; opts_.trim_total = trim_begin_ + trim_end_; }
    void setTrimEndLength(int l) { trim_end_ = l; opts_.trim_total = trim_begin_ + trim_end_; }
    bool setReadLengths(const std::string &s);  // "64", "64-72", "-64", "+64" (filter.cpp:150-183)
    uint64_t kept = 0;
protected:
    int runInternal(ChainContext &cc, ReadBatch &b) override;
    std::string region_;
    bool has_region_ = false;
    struct RegionLine {
        std::string text;
        uint64_t line;  // 1-based line of the -L file, 0: from addRegion
    };
    std::vector<RegionLine> more_regions_;
    std::string regions_file_;
    int trim_begin_ = 0, trim_end_ = 0;
    oge_filter_opts opts_;
};

// ReadSorter (algorithms/read_sorter.h:32-105): coordinate sort (oge_sort_coord_dev) or, with
// setSortBy(QUERYNAME), name sort (oge_sort_name_dev) on the GPU, then the permutation gather.  The temp-file knobs are accepted for interface parity; one device sort
// replaces the reference's spilled runs and k-way merge.
class ReadSorter : public AlgorithmModule {
public:
    explicit ReadSorter(const std::string &tmpdir = "/tmp/") : AlgorithmModule("ReadSorter") { (void)tmpdir; }
    void setSortBy(BamHeaderModel::SortOrder o) { order_ = o; }
    void setCompressTempFiles(bool) {}
    void setAlignmentsPerTempfile(int) {}
protected:
    int runInternal(ChainContext &cc, ReadBatch &b) override;
    BamHeaderModel::SortOrder order_ = BamHeaderModel::COORDINATE;
public:
    BamHeaderModel::SortOrder sortBy() const { return order_; }
};

// MarkDuplicates (algorithms/mark_duplicates.h:27-68): -v --nosplit semantics on the GPU.
class MarkDuplicates : public AlgorithmModule {
public:
    explicit MarkDuplicates(const std::string &tmpdir = "/tmp/") : AlgorithmModule("MarkDuplicates") { (void)tmpdir; }
    bool removeDuplicates = false;
    bool compatNonverbose = false;  // reproduce the index bug of runs without -v
    int splitChains = 0;            // > 1 = the result of the split-by-chromosome chains
    uint64_t duplicates = 0;
    // --metrics FILE: Picard's duplication metrics of the marked records (oge_dup_metrics_dev), counted before any
    // removal wherever the marking ran -- in place, fused with the sort, per range of the chunked sort, per rank --
    // and summed here by library id; runChain writes the file (oge_dup_metrics_text) once the chain has run.
    // metricsCommandLine goes into the file's header.
    std::string metricsFilename, metricsCommandLine;
    std::vector<OgeDupMetrics> metrics;       // by library id
    std::vector<std::string> metricsLibraries;  // the ids' names, "" where no @RG names the id
    int metricsUnknown = 0;                     // the id of "Unknown Library"
    double metricsMs = 0;                       // stage dup_metrics, summed over the calls (ranks: the slowest)
    // --optical-distance N (with --metrics; one GPU, records resident in HBM): the duplicate sets of the marked
    // records (oge_dup_sets_dev), taken where the counts are taken in the in-place dedup and the fused sort; the file
    // then carries the optical column and the set-size histogram (oge_dup_sets_text).  -1: not asked for.
    int64_t opticalDistance = -1;
    std::vector<OgeDupSetsLib> sets;            // by library id
    std::vector<uint64_t> setsHist;             // 3 * OGE_DUP_SETS_BINS
    double setsMs = 0;                          // stage dup_sets
    uint64_t setsTiers[3] = {0, 0, 0};          // sets of two or more pairs counted in a wave, in a workgroup, on the host
    int writeMetrics() const;
protected:
    int runInternal(ChainContext &cc, ReadBatch &b) override;
    friend class ReadSorter;
};

// LocalRealignment (algorithms/local_realignment.h:67-527): oge_localrealign (host phases + the
// GPU offset scan).
class LocalRealignment : public AlgorithmModule {
public:
    LocalRealignment() : AlgorithmModule("LocalRealignment") {}
    bool verbose = false;
    void setReferenceFilename(const std::string &f) { reference_ = f; }
    void setIntervalsFilename(const std::string &f) { intervals_ = f; }
    // --auto-targets: the intervals are computed from the batch (oge_targets_dev at its defaults) and handed to the
    // realigner through a file in tmpdir that is removed afterwards; no targets: the records pass through
    void setAutoTargets(bool on, const std::string &tmpdir) { auto_targets_ = on; tmpdir_ = tmpdir; }
protected:
    int runInternal(ChainContext &cc, ReadBatch &b) override;
    int auto_targets(ChainContext &cc, ReadBatch &b, std::string &path, uint64_t *n_targets);
    std::string reference_, intervals_, tmpdir_ = "/tmp";
    bool auto_targets_ = false;
};

// CalMD (`openge calmd`, `localrealign --calmd`; not in the reference, whose users follow it with `samtools calmd`):
// the NM and MD tags of the batch recomputed against the reference FASTA on the GPU.  The batch goes to the device
// if it is not there, one oge_calmd_dev call rewrites it, and the batch's device form is replaced by a copy of the
// call's output (which belongs to the context).  One GPU; a batch that does not fit in HBM beside its output and
// the reference is refused.
class CalMD : public AlgorithmModule {
public:
    CalMD() : AlgorithmModule("CalMD") {}
    void setReferenceFilename(const std::string &f) { reference_ = f; }
    oge_calmd_result result{};
    // before anything is read: false (with a message) when the inputs' files alone, twice over, and the FASTA
    // exceed the free device memory -- the records and their rewritten copy are at least as large as the files
    static bool fitsDevice(ChainContext &cc, const std::vector<std::string> &inputs, const std::string &reference);
protected:
    int runInternal(ChainContext &cc, ReadBatch &b) override;
    std::string reference_;
};

// The multi-GPU form of ReadSorter (+ MarkDuplicates) and of a standalone MarkDuplicates: the batch
// is cut into G contiguous input ranges, one per rank, and oge_sort_markdup_dist leaves b.slices.  With `metrics`
// (n_lib entries, added to) every rank counts its own output slice and the host sums; *metrics_ms += the slowest
// rank's stage time.
int run_ranks(ChainContext &cc, ReadBatch &b, bool sort, const oge_markdup_opts *opts, uint64_t *n_dup,
              std::vector<OgeDupMetrics> *metrics = nullptr, double *metrics_ms = nullptr);

// FileWriter (algorithms/file_writer.cpp:45-196): BAM output, @PG record unless --nopg, BGZF at the
// given level, bin recomputed on every record; SAM text, and FASTQ text to stdout, formatted on the device
// (write_text).  The reference's RAWBAM and CRAM formats, and FASTQ to files, are refused.
enum FileFormat { FORMAT_BAM, FORMAT_RAWBAM, FORMAT_SAM, FORMAT_CRAM, FORMAT_FASTQ, FORMAT_UNKNOWN };
// detectFileFormatFromFilename (util/file_io.h:30-47): by the lower-cased name's suffix
FileFormat detect_file_format(std::string name);
class FileWriter : public AlgorithmModule {
public:
    FileWriter() : AlgorithmModule("FileWriter") {}
    void setFilename(const std::string &f) { filename_ = f; }
    void setCompressionLevel(int l) { level_ = l; }
    int write_device(ChainContext &cc, ReadBatch &b, BgzfWriter &w, double *t_dev, double *t_d2h, double *t_wait);
    int write_slices(ChainContext &cc, ReadBatch &b, BgzfWriter &w);
    int write_ranges(ChainContext &cc, ReadBatch &b, BgzfWriter &w);
    void addProgramLine(const std::string &cl) { program_line_ = cl; }
    // -F: "bam", "sam" or "fastq" as detect_file_format reads them; anything else prints the reference's
    // message and returns -1
    int setFormat(const std::string &f);
    // `view`: with no -F the output name's suffix decides, then this default (file_writer.cpp:57-67); the other
    // commands write BAM whatever the name
    void setDefaultFormat(FileFormat f) { default_format_ = f; detect_from_name_ = true; }
    FileFormat getFileFormat() const;
    void setTrim(int begin, int end) { trim_begin_ = begin; trim_end_ = end; }  // FASTQ: bases cut from both ends
    // SAM / FASTQ: size pass and scan once, then the emit pass chunk by chunk into a device buffer, each chunk
    // copied into one of two page-locked buffers and written (with the host-formatted lines spliced in) while
    // the next one is formatted.  OGE_TEXT_CHUNK = bytes of text per chunk.
    int write_text(ChainContext &cc, ReadBatch &b, FileFormat fmt);
    // --index: <out>.bai beside the BAM, built on the device from the records write_device compresses
    // (oge_bai_build_dev); only the one-GPU device writer provides it, every other path fails before it writes
    void setIndex(bool on) { index_ = on; }
protected:
    int runInternal(ChainContext &cc, ReadBatch &b) override;
    std::string filename_ = "stdout", program_line_;
    int level_ = 6;
    bool index_ = false;
    FileFormat format_ = FORMAT_UNKNOWN, default_format_ = FORMAT_BAM;
    bool detect_from_name_ = false;
    int trim_begin_ = 0, trim_end_ = 0;
    uint64_t index_hdr_z_ = 0, index_hdr_u_ = 0;  // compressed / decompressed size of the header blocks
    std::vector<uint8_t> bai_;                    // the index image write_device built
};

// `openge index in.bam [-o out.bai]`: the file into HBM, oge_bam_index_dev, the image to out (in.bam.bai)
int index_bam_file(ChainContext &cc, const std::string &path, const std::string &out);

// `openge stats [-I] [-L] in.bam`, `openge count in.bam`, `openge coverage [-o out.tsv] [-b N]
// [--omituncoveredbases] in.bam`: the file into HBM, one whole-file call (oge_bam_stats_dev /
// oge_bam_count_dev / oge_bam_coverage_dev), the reference's text formatted on the host
// (algorithms/statistics.cpp:157-201, algorithms/measure_coverage.cpp:128-181)
int stats_bam_file(ChainContext &cc, const std::string &path, bool inserts, bool lengths);
int count_bam_file(ChainContext &cc, const std::string &path);
int coverage_bam_file(ChainContext &cc, const std::string &path, const std::string &out, int binsize, bool omit_uncovered);

// `openge targets [-o out.intervals] [--maxinterval N] [--gap N] in.bam|in.sam`: the file into HBM through the
// same loader, one call (oge_bam_targets_dev, or oge_targets_dev on the records of a SAM file), the text as the
// device wrote it to out ("stdout": standard output)
int targets_bam_file(ChainContext &cc, const std::string &path, const std::string &out, int max_interval, int gap);

// `openge dupmetrics [-o out.txt] in.bam|in.sam`: the duplication metrics of a file that is already marked, by this
// tool or another: the file into HBM through the same loader, one call (oge_bam_dup_metrics_dev, or
// oge_dup_metrics_dev on the records of a SAM file), the text of oge_dup_metrics_text to out ("stdout": standard output).
// optical_distance >= 0: also the duplicate sets (oge_bam_dup_sets_dev / oge_dup_sets_dev), the text of oge_dup_sets_text
int dupmetrics_bam_file(ChainContext &cc, const std::string &path, const std::string &out, const std::string &command_line,
                        int64_t optical_distance = -1);

// `openge compare [-r REGION]... [-p] ref.bam other.bam [more...]` (commands/command_compare.cpp): every input
// through a FileReader into its own batch in HBM, file 0 resident while the others come and go; the regions
// parsed against file 0's dictionary; one oge_compare_dev call per (file, region); the reference's text formatted
// on the host, the file names on stderr, everything else on stdout
int compare_files(ChainContext &cc, const std::vector<std::string> &inputs, const std::vector<std::string> &regions, bool print);

}  // namespace oge
