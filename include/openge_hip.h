/* openge_hip.h -- C ABI of libopenge_hip.so, the MI355X (gfx950) drop-in for OpenGE's
 * post-alignment hot path: coordinate sort, duplicate marking, local-realignment scoring.
 *
 * Conventions: every entry point returns 0 on success and a negative oge_status on failure
 * (message via oge_last_error); no C++ exceptions cross the ABI; plain pointers and sizes
 * only.  Record buffers hold BAM records exactly as in a decompressed BAM stream
 * (block_size u32 + 32-byte core + variable data, util/bam_deserializer.h:143-193) and are
 * addressed by a u64 byte offset per record.
 *
 * Entry points named *_dev take device (HBM) pointers and run on the context's HIP stream;
 * the others take host buffers and copy in/out.  One context per host thread and GPU.
 *
 * Reference interfaces replaced (paths under openge/src/):
 *   oge_sort_coord*      <- ReadSorter (algorithms/read_sorter.h:32-105, .cpp:48-232) with
 *                           Sort::ByPosition (util/bamtools/Sort.h:116-136) and the
 *                           MultiReader run merge (util/read_stream_reader.h:132-153)
 *   oge_gather_records*  <- BamSerializer::write's record encode incl. bin recompute
 *                           (util/bam_serializer.h:105-147) applied to the sorted stream
 *   oge_markdup*         <- MarkDuplicates::runInternal/buildSortedReadEndLists/
 *                           generateDuplicateIndexes (algorithms/mark_duplicates.cpp:185-475)
 *   oge_realign_scan*    <- LocalRealignment::findBestOffset + mismatchQualitySumIgnoreCigar
 *                           (algorithms/local_realignment.cpp:641-679,1126-1164)
 */
#ifndef OPENGE_HIP_H
#define OPENGE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum oge_status {
    OGE_OK = 0,
    OGE_ERR_ARG = -1,      /* bad argument / malformed record */
    OGE_ERR_HIP = -2,      /* HIP runtime error (no device, launch failure, OOM) */
    OGE_ERR_LIMIT = -3,    /* input outside supported limits */
    OGE_ERR_IO = -4        /* file / codec error */
} oge_status;

typedef struct oge_ctx oge_ctx;

/* ---- context ---------------------------------------------------------------------- */
int oge_ctx_create(int device, oge_ctx **out);
/* number of HIP devices visible to the process (0 when there is none) */
int oge_device_count(void);
/* stream: a hipStream_t (0 = the context's own non-blocking stream) */
int oge_ctx_set_stream(oge_ctx *ctx, void *stream);
void *oge_ctx_stream(oge_ctx *ctx);
int oge_ctx_sync(oge_ctx *ctx);
void oge_ctx_destroy(oge_ctx *ctx);
const char *oge_last_error(const oge_ctx *ctx);   /* ctx may be NULL (thread-local last error) */
/* last pipeline's kernel timings in ms, measured with HIP events on the context stream */
int oge_ctx_timing(oge_ctx *ctx, const char *stage, double *ms_out);
/* A work count of the context's last pipeline call (e.g. "shard_blocks", "shard_zbytes",
 * "shard_bytes", "shard_records" of oge_bgzf_decode_shard: this rank's BGZF blocks, their compressed
 * and decompressed bytes, its records).  OGE_ERR_ARG when the call recorded no such count. */
int oge_ctx_counter(oge_ctx *ctx, const char *name, uint64_t *value);
/* version string of the library, gfx target it was built for */
const char *oge_version(void);

/* ---- device buffers (for host code that stages records in HBM without HIP headers) ---- */
int oge_dev_alloc(oge_ctx *ctx, uint64_t bytes, void **out);
int oge_dev_free(oge_ctx *ctx, void *p);
/* kind: 1 = host->device, 2 = device->host, 3 = device->device, 4 = any (also between two GPUs'
 * HBM); synchronous on the ctx stream */
int oge_memcpy(oge_ctx *ctx, void *dst, const void *src, uint64_t bytes, int kind);
/* enable != 0: device buffers (oge_dev_alloc and the library's workspaces) come from the device's
 * stream-ordered pool and freed memory stays reserved for the next allocation of this process
 * (a module chain then reuses one module's buffers for the next).  Call before any allocation;
 * buffers must be freed with the same setting. */
int oge_ctx_set_pool(oge_ctx *ctx, int enable);
/* Page-locked host memory (DMA at full PCIe rate) for staging compressed output. */
int oge_host_alloc(oge_ctx *ctx, uint64_t bytes, void **out);
int oge_host_free(oge_ctx *ctx, void *p);

/* ---- coordinate sort (ReadSorter + Sort::ByPosition) ------------------------------ */
/* perm_out[k] = input index of the record at sorted position k.  Order: refID ascending with
 * refID == -1 last; pos; forward before reverse; read name bytes; flag; input index (the
 * reference's final tie-break is the record's heap address).  Records with
 * refID == -1 keep input order (reference order there is implementation-defined, Q11).
 * n_ref: number of reference sequences (refIDs must lie in [-1, n_ref)). */
int oge_sort_coord(oge_ctx *ctx, const uint8_t *recs, uint64_t rec_bytes, const uint64_t *rec_off,
                   uint64_t n, int32_t n_ref, uint32_t *perm_out);
int oge_sort_coord_dev(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n,
                       int32_t n_ref, uint32_t *d_perm);

/* ---- permutation gather with BAM re-encode (bin recompute) ------------------------- */
/* out record k = record perm[k] with its bin field recomputed as the reference writer does.
 * d_out_off (n+1 entries) receives the output offsets; d_out must hold the same byte total. */
int oge_gather_records_dev(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, const uint32_t *d_perm,
                           uint64_t n, uint8_t *d_out, uint64_t *d_out_off);

/* Device primitive used by every sort above, exposed for tests: stable LSD radix sort of
 * (u64 key, u32 value) pairs on the key bits in bit_mask (d_vals/d_vtmp may be NULL).  The sorted
 * pairs end in (d_keys, d_vals) when *in_tmp_out == 0, in (d_ktmp, d_vtmp) when 1. */
int oge_radix_sort_pairs_dev(oge_ctx *ctx, uint64_t *d_keys, uint32_t *d_vals, uint64_t *d_ktmp, uint32_t *d_vtmp,
                             uint64_t n, uint64_t bit_mask, int *in_tmp_out);

/* Device primitive behind every compaction and offset table, exposed for tests: exclusive prefix sum
 * of n unsigned elements of elem_bytes (4 or 8) bytes, d_out may equal d_in.  Synchronous. */
int oge_exclusive_scan_dev(oge_ctx *ctx, const void *d_in, void *d_out, uint64_t n, int elem_bytes);

/* ---- duplicate marking (MarkDuplicates) ------------------------------------------- */
typedef struct oge_markdup_opts {
    int32_t n_ref;
    /* Read-group -> library table: rg_ids is n_rg NUL-terminated IDs back to back; rg_lib[i] is
     * the library id (>= 1) of rg i.  Records whose RG is absent / unknown / has no LB use
     * unknown_lib (getLibraryName, algorithms/mark_duplicates.cpp:301-318). */
    const char *rg_ids;
    uint64_t rg_ids_bytes;
    const int16_t *rg_lib;
    int32_t n_rg;
    int16_t unknown_lib;
    /* Test knob: 1 = group fragments / pairs with the sort-based stages even where the windowed
     * ones apply (records in sorted order on one GPU).  Results must not change. */
    int16_t debug_sort_groups;
    /* Reproduce the reference's non-verbose index bug: the record index only
     * advances under -v, so every ReadEnds carries index 0.  Default 0 = -v semantics. */
    int32_t compat_nonverbose_index;
    /* 1 = drop duplicates from the output (-r/-R); affects oge_markdup's n_kept only */
    int32_t remove_duplicates;
    /* Test knob: keep only this many bits (1..47) of the 48-bit pair-key hash, to force the
     * collision paths of the mate join.  0 = full hash.  Results must not change. */
    int32_t debug_hash_bits;
    /* Split-by-chromosome emulation (cmd/command_dedup.cpp:71-106,
     * algorithms/split_by_chromosome.cpp:45-48): K > 1 gives the result of K MarkDuplicates chains
     * fed refID % K (refID < 0 -> chain 0) -- mates in different chains never pair.  The
     * reference's default when --nosplit is absent, with K = min(12, threads / 2).  0 or 1 =
     * --nosplit.  Not combinable with compat_nonverbose_index. */
    int32_t split_chains;
} oge_markdup_opts;

/* dup_out[i] (per input record, input order = record index): 1 if record i is flagged
 * 0x400, 0 if a primary record that gets 0x400 cleared, 2 if non-primary (flag untouched).
 * flags_out (optional, may be NULL): the record's new FLAG field. */
int oge_markdup(oge_ctx *ctx, const uint8_t *recs, uint64_t rec_bytes, const uint64_t *rec_off, uint64_t n,
                const oge_markdup_opts *opts, uint8_t *dup_out, uint64_t *n_dup_out);
/* Device form: also rewrites FLAG 0x400 in place in d_recs when apply != 0. */
int oge_markdup_dev(oge_ctx *ctx, uint8_t *d_recs, const uint64_t *d_off, uint64_t n,
                    const oge_markdup_opts *opts, uint8_t *d_dup, int apply, uint64_t *n_dup_out);

/* ---- fused sort + markdup (mergesort -M --nosplit) on device-resident records -------- */
/* d_out/d_out_off receive the sorted records with bin recomputed and 0x400 applied.
 * d_perm (n) receives the permutation. */
int oge_sort_markdup_dev(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n,
                         const oge_markdup_opts *opts, uint32_t *d_perm, uint8_t *d_out, uint64_t *d_out_off,
                         uint64_t *n_dup_out);

/* Allocate the mergesort chain's two record arenas for streams of up to `total` decompressed bytes now
 * (a long-running caller reserves them once; HBM re-acquired inside a call is wiped by the driver first,
 * ~35-45 GB/s).  *x / *y (cap bytes each) may hold the caller's data between chain calls. */
int oge_mergesort_reserve(oge_ctx *ctx, uint64_t total, void **x, void **y, uint64_t *cap);

/* ---- the whole mergesort chain on a BAM file resident in HBM -------------------------- */
/* FileReader -> ReadSorter -> [MarkDuplicates] -> FileWriter as MergeSortCommand::runCommand wires
 * it (commands/command_mergesort.cpp:68-117), every stage on the device: BGZF framing index,
 * inflate + CRC check, record walk, coordinate sort (+ duplicate marking, -M), optional removal
 * (-R), header regeneration (SO:coordinate, @PG unless program_line is NULL = --nopg), BGZF
 * deflate, EOF block.  d_z = the whole input file (4-byte aligned).  On success *d_out points at
 * the whole output BAM file in HBM, valid until the next call on ctx. */
typedef struct oge_mergesort_opts {
    int32_t level;                   /* output BGZF level 0..9 (FileWriter -c; default 6) */
    int32_t mark_duplicates;         /* -M */
    int32_t remove_duplicates;       /* -R (with -M) */
    int32_t compat_nonverbose_index; /* oge_markdup_opts field of the same name */
    int32_t split_chains;            /* oge_markdup_opts field of the same name */
    int32_t build_index;             /* != 0: oge_mergesort_bgzf_dev also builds the .bai of the file it returns
                                      * (fetch it with oge_ctx_last_bai).  oge_mergesort_bgzf_host / _dist / _shard
                                      * fail with OGE_ERR_ARG ("index not provided on this path") when it is set. */
    const char *program_line;        /* @PG CL, or NULL (--nopg) */
} oge_mergesort_opts;
void oge_mergesort_opts_init(oge_mergesort_opts *o);
int oge_mergesort_bgzf_dev(oge_ctx *ctx, const uint8_t *d_z, uint64_t zbytes, const oge_mergesort_opts *o,
                           const uint8_t **d_out, uint64_t *out_bytes, uint64_t *n_reads, uint64_t *n_dup);
/* The same chain on a BAM file in HOST memory with the PCIe transfers overlapped (replaces the reader and
 * writer threads of BgzfInputStream / BgzfOutputStream, util/bgzf_input_stream.cpp:180-206,
 * util/bgzf_output_stream.cpp:252-285): h_z goes up in chunks on a copy stream while the host indexes its
 * framing and the chunks already up are inflated; after the sort the output is deflated in block-aligned
 * segments whose copies down into h_out (out_cap bytes) run on a high-priority stream while the next
 * segment is compressed (OGE_HOSTPIPE_DIRECT=1 with a page-locked h_out of header + oge_bgzf_bound + 28
 * bytes: the deflate writes straight into h_out instead).  The output bytes equal
 * oge_mergesort_bgzf_dev's.  h_z and h_out should be page-locked (oge_host_alloc). */
int oge_mergesort_bgzf_host(oge_ctx *ctx, const uint8_t *h_z, uint64_t zbytes, const oge_mergesort_opts *o, uint8_t *h_out,
                            uint64_t out_cap, uint64_t *out_bytes, uint64_t *n_reads, uint64_t *n_dup);

/* ---- inputs larger than HBM (replaces ReadSorter's spilled runs + k-way merge) ---------- */
/* Receives one output range: n records in HBM (d_off: n + 1 offsets from d_recs), valid during the
 * call; ranges arrive in output order.  Non-zero return aborts the sort with that status. */
typedef int (*oge_range_cb)(void *user, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n);
/* mergesort [-M] of records in HOST memory of any size on one GPU (alg/read_sorter.cpp:48-190,
 * util/read_stream_reader.h:132-153): sorted runs of <= chunk_bytes (0 = sized from free HBM) are
 * written back over the input arena (h_recs is the spill space and holds the runs afterwards;
 * h_off[0..n] is read-only), key ranges that fit HBM are cut from the runs and sorted on the device,
 * and with opts != NULL the duplicate marks of the whole input are computed on a device-resident
 * summary array first (64 B/read + ~140 B/read of scratch).  Output = oge_sort_markdup_dev's, handed
 * to cb range by range.  *n_runs / *n_ranges (optional) report the cut. */
int oge_sort_markdup_chunked(oge_ctx *ctx, uint8_t *h_recs, const uint64_t *h_off, uint64_t n, int32_t n_ref,
                             const oge_markdup_opts *opts, uint64_t chunk_bytes, oge_range_cb cb, void *user,
                             uint64_t *n_dup, uint64_t *n_runs, uint64_t *n_ranges);
/* free / total bytes of the context's device memory */
int oge_mem_info(oge_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes);

/* ---- multi-GPU sort + duplicate marking (replaces SplitByChromosome / SortedMerge) ------ */
/* One rank per GPU.  The reference parallelises mergesort -M / dedup by routing refID % K to K
 * MarkDuplicates chains and re-merging them (alg/split_by_chromosome.cpp:30-58,
 * alg/sorted_merge.cpp:66-101, wired by cmd/command_mergesort.cpp:118-179 and
 * cmd/command_dedup.cpp:70-113); here G ranks split the ByPosition key range with sampled
 * splitters, exchange records over RCCL (xGMI), and mark duplicates exactly (= --nosplit on one
 * GPU) with hash-routed mate-join and pair-group exchanges.  Every call below is collective: all
 * ranks of a communicator make it, in the same order. */
typedef struct oge_comm oge_comm;
/* Communicator id for oge_comm_init_rank (made by one rank, shared by the caller): RCCL's unique id
 * plus a random nonce naming the node-local meeting of ranks that share a GPU. */
uint64_t oge_comm_unique_id_bytes(void);
int oge_comm_unique_id(uint8_t *id_out, uint64_t bytes);
/* One rank per process (or per host thread): rank `rank` of `nranks`, every rank with the same id,
 * concurrently.  Transport (OGE_COMM = auto | rccl | host, default auto): RCCL over xGMI between
 * distinct GPUs; "host" (device -> shared host segment -> device, dist_shm.h) when ranks share a GPU,
 * which RCCL refuses -- so the same bootstrap runs on a one-GPU box.  auto takes RCCL when the
 * process sees >= nranks devices, else compares the ranks' PCI bus ids in the shared segment
 * (OGE_COMM_DIR, default /dev/shm or /tmp; OGE_COMM_STAGE_MB per-rank staging, default 32). */
int oge_comm_init_rank(oge_ctx *ctx, int nranks, int rank, const uint8_t *id, oge_comm **out);
/* The same with the transport chosen by the caller (mode "auto" | "rccl" | "host" | "node"; NULL =
 * OGE_COMM).  In auto mode with fewer visible devices than ranks, the shared-segment meeting is tried
 * only when the launcher says every rank is on this node (LOCAL_WORLD_SIZE / OMPI_COMM_WORLD_LOCAL_SIZE /
 * MPI_LOCALNRANKS == nranks); otherwise RCCL, the only transport that reaches other hosts.  "node" =
 * OGE_COMM's choice with every rank known to be on this node.  The CLI, whose ranks are threads of one
 * process, passes "host" when they share a device, else "node".  RCCL ranks on one node exchange their
 * small host-side values (statuses, counts, splitter samples) through a shared segment instead of a
 * device round trip (OGE_COMM_HOSTX=0: the device round trip). */
int oge_comm_init_rank_mode(oge_ctx *ctx, int nranks, int rank, const uint8_t *id, const char *mode, oge_comm **out);
/* Per-exchange record of the communicator's last oge_sort_markdup_dist / oge_mergesort_bgzf_dist /
 * oge_mergesort_bgzf_shard / oge_bgzf_decode_shard call:
 * a JSON array of {tag, calls, bytes_sent, bytes_recv, bytes_self, ms, device_ms, mode} (bytes to / from
 * other ranks and kept on this rank; host wall time of the collectives, waiting for peers included; RCCL's
 * time on its stream; mode: blocking | side_stream for device exchanges, host_memory | device_round_trip
 * for the host-side allgathers).  Returns the JSON
 * length; writes it (NUL-terminated) when cap > length. */
int64_t oge_comm_stats_json(const oge_comm *comm, char *buf, uint64_t cap);
/* One process, n contexts in one call (test harness): RCCL when the contexts' devices are distinct,
 * else (or with OGE_COMM=local) an in-process hub of device-to-device copies.  out[0..n) receives one
 * communicator per context.  The CLI uses oge_comm_init_rank from one thread per rank instead. */
int oge_comm_init(oge_ctx **ctxs, int n, oge_comm **out);
void oge_comm_destroy(oge_comm *comm);
int oge_comm_rank(const oge_comm *comm);
int oge_comm_size(const oge_comm *comm);
const char *oge_comm_transport(const oge_comm *comm); /* "rccl", "host" or "local" */
/* This rank's shard of the input: contiguous input ranges in rank order (any sizes, empty ones
 * included).  sort != 0 (mergesort [-M]): -> this rank's slice of the globally sorted output, with
 * bin recomputed and, when opts != NULL, 0x400 set/cleared exactly as oge_sort_markdup_dev does on
 * the whole input.  sort == 0 (dedup): the shard keeps its records and their order, marked exactly
 * as oge_markdup_dev marks the whole input (record index = input position).  compat_nonverbose_index
 * is one-GPU only.  Concatenating the slices in rank order gives the one-GPU output.  *d_out /
 * *d_out_off (*n_out + 1 offsets) are owned by the rank's context and valid until its next call;
 * *n_dup_total = 0x400 records over all ranks.  d_off[i] are byte offsets from d_recs. */
/* The whole mergesort [-M] [-R] chain (oge_mergesort_bgzf_dev) over the communicator's ranks: rank g
 * passes its own input BAM file (resident in its HBM; the output header is rank 0's file's, as
 * MultiReader takes the first file's), and *d_out receives rank g's slice of the one output file --
 * rank 0's begins with the header, the last rank's ends with the EOF block, so the slices concatenate
 * in rank order (valid until the rank's next call).  *n_reads_total: records written by all ranks. */
int oge_mergesort_bgzf_dist(oge_comm *comm, const uint8_t *d_z, uint64_t zbytes, const oge_mergesort_opts *o,
                            const uint8_t **d_out, uint64_t *out_bytes, uint64_t *n_reads_total, uint64_t *n_dup_total);
int oge_sort_markdup_dist(oge_comm *comm, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, int32_t n_ref, int sort,
                          const oge_markdup_opts *opts, uint8_t **d_out, uint64_t **d_out_off, uint64_t *n_out,
                          uint64_t *n_dup_total);
/* ONE BGZF BAM file read by every rank from its own byte range (config 4 on the node; replaces the
 * reader thread of BgzfInputStream util/bgzf_input_stream.cpp:180-206 + BamDeserializer::read
 * util/bam_deserializer.h:143-193 feeding SplitByChromosome, cmd/command_mergesort.cpp:118-179).  Rank g
 * holds the file's bytes [a_g, a_g + zbytes) in HBM, a_g = the sum of the earlier ranks' own_bytes, and
 * decodes the BGZF blocks that START in [a_g, a_g + own_bytes): the buffer must hold them whole (own_bytes
 * + 65536 bytes, or up to the end of the file, which the last rank's buffer ends at; zbytes >= own_bytes).
 * The ranks confirm their first block / first record with their predecessors' walk exits (allgathers)
 * and fetch the <= 16 KiB tail of the record that straddles their part's end from the next ranks (an
 * all-to-all).  Out: this rank's records -- those that START in its part of the decompressed stream, in
 * file order, complete in its HBM (*d_off: n + 1 offsets into *d_recs, library workspace valid until the
 * next call on the rank's context) -- and the raw BAM header (rank 0's, shared), copied to hdr_out when
 * hdr_cap holds it (*hdr_len = its length; OGE_ERR_LIMIT otherwise).  The rank shards are contiguous
 * input ranges in rank order: oge_sort_markdup_dist's input.  Collective. */
int oge_bgzf_decode_shard(oge_comm *comm, const uint8_t *d_z, uint64_t zbytes, uint64_t own_bytes, const uint8_t **d_recs,
                          const uint64_t **d_off, uint64_t *n, uint8_t *hdr_out, uint64_t hdr_cap, uint64_t *hdr_len);
/* oge_mergesort_bgzf_dist over ONE input file sharded by byte range as oge_bgzf_decode_shard takes it:
 * every rank inflates ~1/G of the blocks, then the range-split sort + exact dedup, then every rank
 * deflates its slice of the output file (rank 0's with the header, the last rank's with the EOF block). */
int oge_mergesort_bgzf_shard(oge_comm *comm, const uint8_t *d_z, uint64_t zbytes, uint64_t own_bytes, const oge_mergesort_opts *o,
                             const uint8_t **d_out, uint64_t *out_bytes, uint64_t *n_reads_total, uint64_t *n_dup_total);
/* Device synthetic generation of the slot range [slot0, slot0 + nslots) of a data set (one rank's
 * shard of a multi-GPU input). */
int oge_synth_offsets_range_dev(oge_ctx *ctx, const void *params, uint64_t slot0, uint64_t nslots, uint64_t *d_offs);
int oge_synth_records_range_dev(oge_ctx *ctx, const void *params, uint64_t slot0, uint64_t nslots,
                                const uint64_t *d_offs, uint8_t *d_out);

/* ---- local realignment (LocalRealignment) ----------------------------------------- */
/* Offset scan, the realigner's hot loop: for every pair (consensus c, altRead r) the best
 * offset of r on c and its mismatch-quality score, exactly as findBestOffset returns them
 * (algorithms/local_realignment.cpp:1126-1164 over mismatchQualitySumIgnoreCigar :641-679).
 * cons / bases are ASCII bases; quals are raw phred bytes (BAM layout) aligned with bases;
 * pairs holds n_pairs x {cons index, read index, orig offset, maxPossibleStart}. */
typedef struct oge_realign_scan_batch {
    const uint8_t *cons;
    uint64_t cons_bytes;
    const uint64_t *cons_off;   /* n_cons + 1 */
    uint32_t n_cons;
    uint32_t n_reads;
    const uint8_t *bases;
    const uint8_t *quals;
    uint64_t read_bytes;
    const uint64_t *read_off;   /* n_reads + 1 */
    const int32_t *pairs;
    uint64_t n_pairs;
} oge_realign_scan_batch;
int oge_realign_scan(oge_ctx *ctx, const oge_realign_scan_batch *batch, int32_t *best_index, int32_t *best_score);

/* LocalRealignment's tunables (constructor constants, algorithms/local_realignment.cpp:1434-1460) */
typedef struct oge_realign_opts {
    double lod_threshold;            /* 5.0 */
    double mismatch_threshold;       /* 0.15 (entropy) */
    int32_t max_records_in_memory;   /* 150000 */
    int32_t max_isize_for_movement;  /* 3000 */
    int32_t max_pos_move_allowed;    /* 200 */
    int32_t max_reads;               /* 20000 */
    int32_t no_original_alignment_tags;
    int32_t threads;                 /* host threads, 0 = all cores */
} oge_realign_opts;
void oge_realign_opts_init(oge_realign_opts *opts);

/* Whole LocalRealignment module (map_func binning, consensus generation, offset scan on the GPU,
 * LOD / entropy decision, CIGAR + tag updates, ConstrainedMateFixingManager emission) over
 * coordinate-sorted records; replaces LocalRealignment::runInternal
 * (algorithms/local_realignment.cpp:1462-1490) with the writer chain of
 * cmd/command_localrealign.cpp:37-75.  header_text supplies the sequence dictionary. */
typedef struct oge_realign_result oge_realign_result;
int oge_localrealign(oge_ctx *ctx, const char *header_text, uint64_t header_len, const uint8_t *recs,
                     const uint64_t *rec_off, uint64_t n, const char *fasta_path, const char *intervals_path,
                     const oge_realign_opts *opts, oge_realign_result **out);
/* The same over n_ctx devices (realign sharded by interval ranges).  The work intervals are cut
 * into n_ctx contiguous ranges balanced by the reads to clean -- cuts fall inside contigs as well, a
 * single-contig input included -- and device g generates the consensuses of range g and scans their pairs
 * (realign_prep.hip, realign.hip); binning, decisions and the mate-fixing writer run once on the host over
 * the whole input, so the output equals oge_localrealign's for any input and no writer state crosses a cut.
 * Per-device counts are in the result's stats (prep_rank<g>_intervals / _reads / _pairs).  Errors and
 * messages go to ctxs[0]. */
int oge_localrealign_multi(oge_ctx *const *ctxs, int n_ctx, const char *header_text, uint64_t header_len, const uint8_t *recs,
                           const uint64_t *rec_off, uint64_t n, const char *fasta_path, const char *intervals_path,
                           const oge_realign_opts *opts, oge_realign_result **out);
uint64_t oge_realign_result_count(const oge_realign_result *r);
const uint8_t *oge_realign_result_records(const oge_realign_result *r, uint64_t *bytes_out);
const uint64_t *oge_realign_result_offsets(const oge_realign_result *r);   /* count + 1 entries */
const char *oge_realign_result_stats(const oge_realign_result *r);          /* JSON */
void oge_realign_result_free(oge_realign_result *r);

/* ---- synthetic data (bench / tests) ------------------------------------------------ */
/* params: a pointer to oge_synth_params (openge_amd/csrc/synth.h) */
int oge_synth_finalize(void *params);
uint64_t oge_synth_params_size(void);
/* Host generation of slots [0, 2*n_pairs): sizes first (offs gets n+1 prefix offsets), then bytes. */
int oge_synth_offsets_host(const void *params, uint64_t *offs, int threads);
int oge_synth_records_host(const void *params, const uint64_t *offs, uint8_t *out, int threads);
int oge_synth_header_text(const void *params, char *buf, uint64_t cap, uint64_t *len_out);
/* Local-realignment data set (SURVEY §8d C5 shape; openge_amd/csrc/realign_synth.cpp): writes a
 * reference FASTA (+ .fai), a target-interval list and a coordinate-sorted BAM. */
typedef struct oge_realign_synth_params {
    uint64_t seed;
    uint32_t n_ref, n_intervals, spacing, read_len, frags_per_interval;
    uint32_t qual_min, qual_max, ins_min, ins_max;
    uint32_t err_ppm, noindel_ppm, gapped_ppm, alt_indel_ppm, dup_ppm, mapq0_ppm, clip_ppm;
    uint32_t lower_ppm, n_ppm, md_ppm, uq_ppm;
} oge_realign_synth_params;
void oge_realign_synth_defaults(oge_realign_synth_params *p);   /* C5: 50k intervals, 24 contigs */
int oge_synth_realign(const oge_realign_synth_params *p, const char *fasta_path, const char *intervals_path,
                      const char *bam_path, int level, int threads);
/* Device generation straight into HBM. */
int oge_synth_offsets_dev(oge_ctx *ctx, const void *params, uint64_t *d_offs);
int oge_synth_records_dev(oge_ctx *ctx, const void *params, const uint64_t *d_offs, uint8_t *d_out);

/* ---- BAM file helpers (host) -------------------------------------------------------- */
typedef struct oge_bam oge_bam;
int oge_bam_read(const char *path, int threads, oge_bam **out);
void oge_bam_free(oge_bam *b);
uint64_t oge_bam_count(const oge_bam *b);
const uint8_t *oge_bam_records(const oge_bam *b, uint64_t *bytes_out);
const uint64_t *oge_bam_offsets(const oge_bam *b);
int32_t oge_bam_n_ref(const oge_bam *b);
/* regenerated header text (BamHeader::toString, util/bam_header.cpp:184-214) */
int oge_bam_header_text(const oge_bam *b, char *buf, uint64_t cap, uint64_t *len_out);
/* Build the RG -> library table MarkDuplicates derives from the header. Caller frees with free(). */
int oge_bam_markdup_opts(const oge_bam *b, oge_markdup_opts *opts, char **rg_ids_buf, int16_t **rg_lib_buf);
/* Write a BGZF BAM: header from `header_text`, records in the given order (order may be NULL
 * for identity), optional FLAG overrides (flags may be NULL). sort_order: -1 keep, else
 * BamHeader::sort_order_t. */
int oge_bam_write(const char *path, const char *header_text, uint64_t header_len, int sort_order,
                  const uint8_t *recs, const uint64_t *offs, uint64_t n, const uint32_t *order,
                  const uint16_t *flags, int level, int threads);

/* ---- BGZF compression on the device (replaces BgzfOutputStream's deflate workers,
 * util/bgzf_output_stream.cpp:59-250; crc32 at :139) ---------------------------------- */
/* Worst-case size of the BGZF stream for n payload bytes (one 64 KiB slot per 65,280-byte block). */
uint64_t oge_bgzf_bound(uint64_t n);
/* Compress n bytes at d_src into consecutive BGZF blocks (65,280-byte payloads; dynamic-Huffman
 * deflate, or stored blocks for level 0 / incompressible payloads) written back to back at d_dst.
 * No EOF marker is appended.  dst_cap must be >= oge_bgzf_bound(n); *out_bytes = stream size.
 * Levels 1-7: greedy one-candidate parse; 8-9: same-prefix match chains (8 / 32 deep) with lazy
 * matching, ~1 % smaller output at 1.7-3x the time.  Deterministic: the same input gives the same bytes.
 * The match search is the context's (oge_ctx_set_deflate_search, below): OGE_DEFL_FAST, the default,
 * OGE_DEFL_NEAR, OGE_DEFL_SPAN or both; level 0 and the stored-block fallback ignore it. */
int oge_bgzf_deflate_dev(oge_ctx *ctx, const uint8_t *d_src, uint64_t n, int level, uint8_t *d_dst,
                         uint64_t dst_cap, uint64_t *out_bytes);
/* The block writer has two instances: blocks of at most this many bytes (header and footer included) are
 * assembled three workgroups to a CU, larger ones two.  OGE_DEFL_EMIT_CAP (bytes, read per call) lowers
 * the limit, 0 sends every block to the large instance; the bytes written are the same either way.  The
 * counters "defl_emit_small" / "defl_emit_big" (oge_ctx_counter) give a call's blocks per instance. */
uint32_t oge_defl_emit_cap(void);
/* Host-buffer form (uploads, compresses, downloads); dst_cap >= the compressed size. */
int oge_bgzf_deflate(oge_ctx *ctx, const uint8_t *src, uint64_t n, int level, uint8_t *dst, uint64_t dst_cap,
                     uint64_t *out_bytes);
/* The match search of oge_bgzf_deflate[_dev] and of every device writer built on it, two independent
 * bits beside `level` (which keeps choosing depth and lazy matching):
 *   OGE_DEFL_FAST  candidates from the earlier rounds of 1024 positions only, matches end at their
 *                  64-byte segment's edge (the default; its bytes never change with the other modes)
 *   OGE_DEFL_NEAR  also the earliest same-prefix position of a position's own round (the previous BAM
 *                  record's name prefix, flags and tags are usually that near)
 *   OGE_DEFL_SPAN  matches run across segment edges, up to 258 bytes (cut at 32 KiB sub-blocks only)
 * On real reads NEAR | SPAN writes 14 % fewer bytes than FAST at level 6 for ~40 % more deflate
 * time, NEAR alone 10 % fewer for ~13 % more.  A new context has OGE_DEFL_FAST unless
 * the environment variable OGE_DEFLATE_SEARCH = fast | near | span | near+span is set when it is created
 * (any other word fails oge_ctx_create).  set: OGE_ERR_ARG outside 0..3. */
enum { OGE_DEFL_FAST = 0, OGE_DEFL_NEAR = 1, OGE_DEFL_SPAN = 2 };
int oge_ctx_set_deflate_search(oge_ctx *ctx, int search);
int oge_ctx_deflate_search(oge_ctx *ctx);
/* ---- BGZF decompression and BAM record boundaries on the device (replaces BgzfInputStream,
 * util/bgzf_input_stream.cpp:65-142,208-240, and BamDeserializer's record walk,
 * util/bam_deserializer.h:143-193) ------------------------------------------------------ */
/* Host: index the BGZF framing of z.  For each block with a non-empty payload (at most cap):
 * d0/d1 = byte range of its deflate data in z, uoff = payload offset (uoff has cap + 1 entries;
 * uoff[nblk] = total), crc = the stored CRC-32.  Any array may be NULL.  *nblk = block count
 * (OGE_ERR_ARG when it exceeds cap). */
int oge_bgzf_index(const uint8_t *z, uint64_t zbytes, uint64_t *d0, uint64_t *d1, uint64_t *uoff, uint32_t *crc,
                   uint64_t cap, uint64_t *nblk);
/* Device form of oge_bgzf_index for a stream resident in HBM (d_z 4-byte aligned): every byte
 * position is tested for a block header in parallel and the candidates are accepted only when they
 * form the exact block chain from offset 0 to zbytes (otherwise the host walk runs on a copy, with
 * its error messages).  Same outputs and capacity rule as oge_bgzf_index, as device arrays; with every
 * array NULL it only counts (*nblk). */
int oge_bgzf_index_dev(oge_ctx *ctx, const uint8_t *d_z, uint64_t zbytes, uint64_t *d_d0, uint64_t *d_d1,
                       uint64_t *d_uoff, uint32_t *d_crc, uint64_t cap, uint64_t *nblk);
/* Inflate the indexed blocks of d_z (4-byte aligned) into d_out + uoff[i]; d_crc (may be NULL)
 * checks every payload's CRC-32.  Fails with OGE_ERR_IO on corrupt data. */
int oge_bgzf_inflate_dev(oge_ctx *ctx, const uint8_t *d_z, uint64_t zbytes, const uint64_t *d_d0, const uint64_t *d_d1,
                         const uint64_t *d_uoff, const uint32_t *d_crc, uint64_t nblk, uint8_t *d_out);
/* Host, no device: how the inflate cuts nblk blocks into phase-1 launches over `lanes` resident decoder lanes
 * when the workspace holds `budget` blocks and a launch takes at most max_per_lane blocks per lane (0: the
 * build's value).  Every chunk is R * lanes blocks, R = clamp(budget / lanes, 1, max_per_lane), and the last
 * takes the remainder, so the launches run ceil(nblk / lanes) rounds for any budget; balanced != 0: the equal
 * chunks OGE_INFL_PLAN=balanced selects.  Returns the chunk count; the first min(count, cap) sizes go to sizes
 * (may be NULL).  The context counters infl_chunks, infl_rounds and infl_lanes report what a call ran. */
uint64_t oge_infl_plan(uint64_t nblk, uint64_t lanes, uint64_t budget, uint64_t max_per_lane, int balanced,
                       uint64_t *sizes, uint64_t cap);
/* Host-buffer form: the whole BGZF stream z -> out (out_cap >= payload total). */
int oge_bgzf_inflate(oge_ctx *ctx, const uint8_t *z, uint64_t zbytes, uint8_t *out, uint64_t out_cap,
                     uint64_t *out_bytes);
/* Record boundaries of the decompressed BAM stream d_stream[rec_base, end): d_off[i] = absolute
 * offset of record i, d_off[n] = end (cap >= n + 1; d_off NULL = count only).  Equals the sequential
 * block_size walk; block_size outside [32, 10000] or a record past the end fails (OGE_ERR_IO). */
int oge_bam_record_offsets_dev(oge_ctx *ctx, const uint8_t *d_stream, uint64_t rec_base, uint64_t end, int32_t n_ref,
                               uint64_t *d_off, uint64_t cap, uint64_t *n_out);
/* Recompute every record's bin field in place (BamSerializer::write, util/bam_serializer.h:112-116). */
int oge_fix_bins_dev(oge_ctx *ctx, uint8_t *d_recs, const uint64_t *d_off, uint64_t n);
/* Copy the records whose FLAG has none of flag_mask set, in order, to d_out / d_out_off (n_out
 * records): the writer side of -r/-R (MarkDuplicates::runInternal, mark_duplicates.cpp:456-458). */
int oge_drop_flagged_dev(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, uint16_t flag_mask,
                         uint8_t *d_out, uint64_t *d_out_off, uint64_t *n_out);

/* ---- BAM index (.bai, SAM v1 section 5.2) of coordinate-sorted records, built on the device ---------
 * The reference writes no index (util/bam_index.cpp:245-246 returns at once); the image is one canonical
 * byte string per input: a chunk is a maximal run of consecutive records with one
 * (refID, bin), chunks of a bin stay in file order and merge when the next starts in the compressed block
 * its predecessor ends in (or an earlier one), bins ascend, pseudo-bin 37450 comes last, nothing is promoted
 * to parent bins, and empty linear windows take the next window's offset.  Not byte-equal to samtools'
 * index, and valid for every BAI reader.
 * Records d_recs + d_off[i] (n offsets), contiguous as in the stream; record 0 sits at decompressed-stream
 * position stream_base.  Block table: d_uoff / d_cstart hold nblk + 1 entries, payload offset and file offset
 * of every block, entry nblk = payload total / the file offset just past the last data block.  Input must be
 * in the project's coordinate order (refID ascending with -1 last, pos ascending): the first violation fails
 * with OGE_ERR_ARG naming the record index; a record that ends past 2^29, or n_ref < 0, with OGE_ERR_LIMIT.
 * *d_bai (device) is valid until the next call on ctx.  Stage name for oge_ctx_timing: "bai_build". */
int oge_bai_build_dev(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, int32_t n_ref,
                      uint64_t stream_base, const uint64_t *d_uoff, const uint64_t *d_cstart, uint64_t nblk,
                      const uint8_t **d_bai, uint64_t *bai_bytes);
/* Host-buffer form (uploads, builds, downloads into out when cap holds it; *bai_bytes = the image size,
 * OGE_ERR_LIMIT when cap is smaller). */
int oge_bai_build(oge_ctx *ctx, const uint8_t *recs, uint64_t rec_bytes, const uint64_t *rec_off, uint64_t n,
                  int32_t n_ref, uint64_t stream_base, const uint64_t *uoff, const uint64_t *cstart, uint64_t nblk,
                  uint8_t *out, uint64_t cap, uint64_t *bai_bytes);
/* A whole BAM file resident in HBM (4-byte aligned) -> its index: framing index, inflate, header, record
 * walk, build.  Blocks with an empty payload are not part of the block table. */
int oge_bam_index_dev(oge_ctx *ctx, const uint8_t *d_z, uint64_t zbytes, const uint8_t **d_bai, uint64_t *bai_bytes);
/* The index the context's last oge_bai_build* / oge_bam_index_dev / oge_mergesort_bgzf_dev(build_index) call
 * built; OGE_ERR_ARG when there is none. */
int oge_ctx_last_bai(oge_ctx *ctx, const uint8_t **d_bai, uint64_t *bai_bytes);

/* ---- reading a BAM index: the ranges of the file that a list of regions needs ------
 * oge_bai_open takes the bytes of any valid .bai (bins in any order, n_no_coor present or not; not only this
 * project's canonical form), checks every length in it against the image on the host and puts it into HBM with
 * a sorted bin directory.  OGE_ERR_ARG, before anything is launched or allocated on the device: no magic, a
 * truncated image, bytes behind the last section, a bin number above 37450, n_ref != n_ref_expected (the BAM
 * header's; < 0: not compared).  The handle belongs to ctx and is released with oge_bai_close (NULL allowed). */
typedef struct oge_bai oge_bai;
int oge_bai_open(oge_ctx *ctx, const uint8_t *bai, uint64_t bytes, int32_t n_ref_expected, oge_bai **out);
void oge_bai_close(oge_bai *bai);
/* The virtual-offset ranges that hold every record overlapping one of the regions (a host array; oge_region is
 * declared with the Filter below).  Region g asks for the reference positions [max(0, left_pos - widen),
 * min(right_pos + 1, 2^29)) of ref_id: the chunks of the bins of that interval (reg2bins, SAM v1 section 5.3), each
 * cut at the linear index entry of the interval's first 16 Ki window.  A region that is empty, whose ref_id is
 * outside [0, n_ref), whose first window lies past the reference's last one or whose reference has no bins asks
 * for nothing.  widen >= 0 reaches back for records that start before left_pos (their l_seq is not what the index
 * was built from).
 * Result: the UNION of all those half-open intervals [beg, end) of virtual offsets -- overlapping and touching
 * ones joined, empty ones dropped, ascending -- as *n_ranges pairs (beg, end) at *d_ranges (device), valid until
 * the context's next query; NULL and 0 when there is none.  Counter "baiq_ranges" = *n_ranges.  Everything else
 * the call allocates is released before it returns.  OGE_ERR_LIMIT: more than 2^23 regions, or 2^32 - 2 ranges
 * before the merge.  Stage name for oge_ctx_timing: "bai_query". */
struct oge_region;
int oge_bai_query_dev(oge_ctx *ctx, const oge_bai *bai, const struct oge_region *regions, uint64_t n_regions, int32_t widen,
                      const uint64_t **d_ranges, uint64_t *n_ranges);
/* Host-buffer form: the pairs into out (cap pairs; OGE_ERR_LIMIT with *n_ranges set when there are more). */
int oge_bai_query(oge_ctx *ctx, const oge_bai *bai, const struct oge_region *regions, uint64_t n_regions, int32_t widen,
                  uint64_t *out, uint64_t cap, uint64_t *n_ranges);
/* The records of the ranges a query returned, decoded from the parts of the file that hold them.  d_z (device,
 * 4-byte aligned, zbytes bytes) holds n_spans spans of the file back to back, each a run of whole BGZF blocks,
 * so d_z is a BGZF stream of its own: span s is the file's bytes [span_file[s], span_file[s] + span_z[s + 1] -
 * span_z[s]) at d_z + span_z[s] (host arrays; span_z has n_spans + 1 entries, span_z[0] = 0, span_z[n_spans] =
 * zbytes; the spans ascend in the file and do not overlap).  d_ranges: n_ranges (beg, end) pairs as
 * oge_bai_query_dev returns them (device), each beginning and ending in a block of the spans; an end may be the
 * first byte behind its span.  The spans are indexed and inflated with one block table, every range's payload
 * bytes are copied into one arena back to back (the chunks of an index are whole records, so the arena is a
 * record stream) and the record walk of oge_bam_record_offsets_dev runs over it once.
 * *d_recs / *d_off (*n + 1 offsets from *d_recs, *rec_bytes bytes of records, 64 zero bytes of slack behind them)
 * are the caller's, to be released with oge_dev_free (NULL when there is no record); everything else the call
 * allocates is released before it returns.  OGE_ERR_ARG: a range that does not begin at
 * the first byte of a block of the spans or reaches past its payload, spans that are not whole blocks;
 * OGE_ERR_IO: corrupt blocks, or a packed stream that the walk does not consume exactly (a refID outside
 * [-1, n_ref) included).  Counter "baiq_blocks": the blocks inflated.  Stage name for oge_ctx_timing:
 * "ranges_pack" (positions, scan and copy); the inflate and the walk report under their own names. */
int oge_bam_decode_ranges_dev(oge_ctx *ctx, const uint8_t *d_z, uint64_t zbytes, const uint64_t *span_z,
                              const uint64_t *span_file, uint64_t n_spans, const uint64_t *d_ranges, uint64_t n_ranges,
                              int32_t n_ref, uint8_t **d_recs, uint64_t **d_off, uint64_t *n, uint64_t *rec_bytes);

/* ---- stats, count and coverage of records in HBM (openge stats / count / coverage) ------------------
 * The reference's Statistics and MeasureCoverage modules (algorithms/statistics.cpp,
 * algorithms/measure_coverage.cpp) as reductions on the device; DESIGN.md section 20.  len = l_seq.
 * Counters: mapped = !(flag & 4); forward / reverse by flag & 0x10; failed_qc 0x200; duplicates 0x400;
 * paired = flag & 1; and only among paired reads proper_pair (flag & 2), read1 (0x40), read2 (0x80),
 * both_mapped (mapped and !(flag & 8)) and singletons (mapped and flag & 8).
 * sorted: only records with refID != -1 and pos != -1 are considered, last_rid = last_pos = -1 at the start;
 * a lower refID than last_rid means unsorted; a higher one sets last_rid and resets last_pos to -1 WITHOUT
 * recording this record's position; an equal one with pos < last_pos means unsorted, else last_pos = pos.
 * So the first considered record of every refID run is exempt as a predecessor: positions 100, 50, 60 on
 * one contig are "sorted", 100, 150, 60 are not.
 * Inserts: over records that are paired, first mate and have tlen != 0, n_insert = their number and
 * insert_sum = the sum of |tlen| (always filled; |INT32_MIN| counts as 2^31); with OGE_STATS_INSERTS
 * insert_mid_lo / insert_mid_hi are the order statistics of |tlen| at ranks (n_insert - 1) / 2 and
 * n_insert / 2 (the median is their mean), both 0 when n_insert is 0.
 * Lengths: with OGE_STATS_LENGTHS, n_lengths and the distinct l_seq values (taken as unsigned) in
 * ascending order with their counts. */
typedef struct oge_bam_stats {
    uint64_t reads, mapped, forward, reverse, failed_qc, duplicates, paired, proper_pair, read1, read2, both_mapped,
        singletons;
    int32_t sorted; /* 1 / 0 */
    int32_t pad0;
    uint64_t n_insert, insert_sum, insert_mid_lo, insert_mid_hi;
    uint64_t n_lengths;
} oge_bam_stats;
enum { OGE_STATS_INSERTS = 1, OGE_STATS_LENGTHS = 2 };
/* Records d_recs + d_off[i] (n offsets; the arena carries 16 bytes of slack behind the last record).
 * *d_len / *d_len_count (device, n_lengths entries, only with OGE_STATS_LENGTHS; may be NULL otherwise) are
 * valid until the next call on ctx.  Stage name for oge_ctx_timing: "qc_stats". */
int oge_stats_dev(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, uint32_t want,
                  oge_bam_stats *stats, const uint32_t **d_len, const uint64_t **d_len_count);
/* Host-buffer form: uploads, reduces, copies the length pairs into len_out / len_count_out (cap entries each;
 * OGE_ERR_LIMIT with *stats filled when n_lengths > cap, so a first call with cap 0 sizes the arrays). */
int oge_stats(oge_ctx *ctx, const uint8_t *recs, uint64_t rec_bytes, const uint64_t *rec_off, uint64_t n, uint32_t want,
              oge_bam_stats *stats, uint32_t *len_out, uint64_t *len_count_out, uint64_t cap);
/* Coverage: contig r has ceil(ref_len[r] / binsize) u32 bins, contiguous in header order:
 * base[r] = the bins of the contigs before it, base[n_ref] = all (base has n_ref + 1 entries).
 * OGE_ERR_ARG when binsize < 1 or n_ref < 0. */
int oge_coverage_layout(int32_t n_ref, const int32_t *ref_len, int32_t binsize, uint64_t *base);
/* Every record with refID != -1 and pos != -1 is counted, FLAG 0x4 reads placed at their mate included; the
 * others add to *n_skipped.  For each of the l_seq + 1 positions i = pos .. pos + l_seq (the query length,
 * not the CIGAR span) bin i / binsize of the contig gains 1.  A position below 0 or in a bin past the
 * contig's last one is dropped (the reference writes outside its vector there).  *overflow = 1 when a bin
 * reached 2^32 - 1; its value is then unspecified.  ref_len is a host array.  OGE_ERR_ARG: binsize < 1, a
 * refID outside [-1, n_ref); OGE_ERR_LIMIT (the message names --binsize): the bins do not fit in free device
 * memory.  *d_bins (device, base[n_ref] entries) is valid until the next call on ctx.  Stage name for
 * oge_ctx_timing: "qc_coverage". */
int oge_coverage_dev(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, int32_t n_ref,
                     const int32_t *ref_len, int32_t binsize, const uint32_t **d_bins, uint64_t *n_skipped,
                     int32_t *overflow);
/* Host-buffer form; bins_out holds cap entries (OGE_ERR_LIMIT when the layout needs more). */
int oge_coverage(oge_ctx *ctx, const uint8_t *recs, uint64_t rec_bytes, const uint64_t *rec_off, uint64_t n,
                 int32_t n_ref, const int32_t *ref_len, int32_t binsize, uint32_t *bins_out, uint64_t cap,
                 uint64_t *n_skipped, int32_t *overflow);
/* A whole BAM file resident in HBM (4-byte aligned): framing index, inflate, header, record walk, then the
 * reduction.  oge_bam_coverage_dev also fails with OGE_ERR_ARG when two contigs share a name; *n_bins =
 * base[n_ref].  oge_bam_count_dev: the number of records. */
int oge_bam_stats_dev(oge_ctx *ctx, const uint8_t *d_z, uint64_t zbytes, uint32_t want, oge_bam_stats *stats,
                      const uint32_t **d_len, const uint64_t **d_len_count);
int oge_bam_coverage_dev(oge_ctx *ctx, const uint8_t *d_z, uint64_t zbytes, int32_t binsize, const uint32_t **d_bins,
                         uint64_t *n_bins, uint64_t *n_skipped, int32_t *overflow);
int oge_bam_count_dev(oge_ctx *ctx, const uint8_t *d_z, uint64_t zbytes, uint64_t *n_reads);
/* The binary reference list (names and lengths, header order) of the file the context's last oge_bam_stats_dev /
 * oge_bam_coverage_dev / oge_bam_count_dev call parsed: *names holds the n_ref names one after the other, each
 * NUL-terminated, *names_bytes bytes in all.  Host pointers, valid until the next such call; OGE_ERR_ARG when
 * there is none. */
int oge_ctx_last_refs(oge_ctx *ctx, int32_t *n_ref, const char **names, uint64_t *names_bytes, const int32_t **ref_len);

/* ---- read-placement diff of two record sets in HBM (openge compare) ---------------------------------
 * The reference's CompareCommand (commands/command_compare.cpp) as a multiset difference on the device;
 * DESIGN.md section 23.  Set a is the reference set ("file 0"), set b the one compared with it.
 * Element of a record: (refID, pos, CIGAR ops), pos the raw 0-based BAM position, each op (length, type char).
 * Two elements are equal when all of it is equal.  Their order (the reference's operator<, the order of the
 * printed diff): refID, pos, the number of ops, then op by op the length (unsigned) and the type CHARACTER,
 * '=' < 'D' < 'H' < 'I' < 'M' < 'N' < 'P' < 'S' < 'X'.
 * Region: a record belongs when left_ref <= refID <= right_ref and left_pos <= pos <= right_pos: the start
 * position alone, both ends inclusive (not the overlap test of oge_filter_records_dev).  "No region" is
 * (0, 0, INT32_MAX, INT32_MAX): refID -1 and pos -1 never belong to it.
 * Counts (64-bit; the reference's are int): n_ref / n_other = the records of a / b inside the region, common =
 * the multiset intersection (the sum over distinct elements of the smaller multiplicity), additions =
 * n_other - common, deletions = n_ref - common.  hard_runs = runs of equal (refID, pos, op count, hash) that
 * held two different CIGARs and were resolved by comparing the ops alone; the counts never depend on the hash.
 * debug_hash_bits (tests): < 0 or >= 47 the full hash, else that many bits (0: every such run is decided by
 * the ops alone).
 * OGE_ERR_ARG (the message names the record): a record inside the region with refID outside [0, n_ref), with a
 * CIGAR op code above 8, or whose CIGAR does not fit its block_size.  OGE_ERR_LIMIT: n_a + n_b >= 2^32 - 1.
 * Diff image (want & OGE_COMPARE_DIFF; diff_entries entries, *diff_bytes bytes, any order, little-endian):
 *   i32 refID, i32 pos, u64 surplus, u32 side (1: set b holds `surplus` more of the element than set a, an
 *   addition; 0: set a holds more, a deletion), u32 n_ops, u32 ops[n_ops] as in the record (len << 4 | code)
 * one entry per element whose multiplicities differ.  *d_diff (device) is valid until the next call on ctx.
 * Stage name for oge_ctx_timing: "compare". */
typedef struct oge_compare_region {
    int32_t left_ref, left_pos, right_ref, right_pos;
} oge_compare_region;
typedef struct oge_compare_result {
    uint64_t n_ref, n_other, common, additions, deletions, diff_entries, hard_runs;
} oge_compare_result;
enum { OGE_COMPARE_DIFF = 1 };
/* Records d_recs_x + d_off_x[i] (n_x offsets; the arenas carry 16 bytes of slack behind the last record);
 * n_ref = the number of contigs of set a's dictionary.  d_diff / diff_bytes may be NULL without OGE_COMPARE_DIFF. */
int oge_compare_dev(oge_ctx *ctx, const uint8_t *d_recs_a, const uint64_t *d_off_a, uint64_t n_a, const uint8_t *d_recs_b,
                    const uint64_t *d_off_b, uint64_t n_b, int32_t n_ref, const oge_compare_region *region, uint32_t want,
                    int debug_hash_bits, oge_compare_result *result, const uint8_t **d_diff, uint64_t *diff_bytes);
/* Host-buffer form: uploads both sets, compares, copies the image into diff_out (cap bytes; OGE_ERR_LIMIT with
 * *result and *diff_bytes filled when the image is larger, so a first call with cap 0 sizes the buffer). */
int oge_compare(oge_ctx *ctx, const uint8_t *recs_a, uint64_t rec_bytes_a, const uint64_t *rec_off_a, uint64_t n_a,
                const uint8_t *recs_b, uint64_t rec_bytes_b, const uint64_t *rec_off_b, uint64_t n_b, int32_t n_ref,
                const oge_compare_region *region, uint32_t want, int debug_hash_bits, oge_compare_result *result,
                uint8_t *diff_out, uint64_t cap, uint64_t *diff_bytes);

/* ---- realignment target intervals of records in HBM (openge targets, localrealign --auto-targets) --------
 * The intervals oge_localrealign takes as its intervals file, computed from the reads' own indels: GATK's
 * RealignerTargetCreator at its defaults without mismatch-entropy events and known indels (the reference has no
 * such step, algorithms/local_realignment.cpp:75-100); DESIGN.md section 25.  Coordinates are 1-based and closed.
 * Reads used: FLAG has none of 0x4, 0x100, 0x200, 0x400; MAPQ is neither 0 nor 255; refID >= 0 and pos >= 0; not
 * a bad mate (FLAG 0x1 set, 0x8 clear, mate refID != refID).
 * Events: first / last = the read's first and last M, = or X op (none: no event); every I or D op at an index
 * strictly between them is an event at a = pos + the lengths of the M, D, N, = and X ops before it (pos the raw
 * 0-based BAM position, so a is the 1-based base just before the indel): an insertion gives (refID, a, a + 1), a
 * deletion of length L (refID, a, a + L); adjacent I and D ops both count, N and P never.  The stop is clipped to
 * the contig's length (a length below 0 counts as 0); a is computed in 64 bits and stored as min(a, 2^31 - 1).
 * Merge: the events in (refID, start, stop) order; an event joins the current interval when it has its refID and
 * start <= the interval's stop + gap, the stop becomes the larger one; otherwise it opens an interval.  n_events
 * = the events that joined.  Drop: an interval with stop - start >= max_interval is left out and counted.
 * Output: the kept intervals in (refID, start) order as oge_target records and, with OGE_TARGETS_TEXT, as lines
 * "contig:start-stop\n" (always both numbers: what the realigner's intervals parser reads).  The order of the
 * input records does not matter.
 * Result: reads_used, events, intervals (before the drop), dropped_long, targets (= intervals - dropped_long),
 * text_bytes (0 without OGE_TARGETS_TEXT).
 * OGE_ERR_ARG (the message names the lowest such record, and of that record the first of the three): a read that
 * passes the filter with refID >= n_ref, with a CIGAR that does not fit its block_size, or with a CIGAR op code
 * above 8; max_interval < 1, gap < 0, n_ref < 0, unknown want bits, names that are not n_ref NUL-terminated
 * strings.  OGE_ERR_LIMIT: events >= 2^32 - 1.
 * Counters (oge_ctx_counter): "targets_tile_records" = the records one workgroup of the event pass takes per
 * append, "targets_merge_tile" = the sorted events one workgroup of the running maximum takes, "targets_events".
 * Stage name for oge_ctx_timing: "targets"; nested in it "targets_count", "targets_events", "targets_sort",
 * "targets_merge" (with the drop and the compaction) and "targets_text". */
typedef struct oge_targets_opts {
    int32_t max_interval; /* 500 (GATK's maxIntervalSize) */
    int32_t gap;          /* 0: touching or overlapping events merge */
    uint32_t want;        /* OGE_TARGETS_TEXT */
} oge_targets_opts;
void oge_targets_opts_init(oge_targets_opts *o);
typedef struct oge_targets_result {
    uint64_t reads_used, events, intervals, dropped_long, targets, text_bytes;
} oge_targets_result;
typedef struct oge_target {
    int32_t ref_id, start, stop;
    uint32_t n_events;
} oge_target;
enum { OGE_TARGETS_TEXT = 1 };
/* Records d_recs + d_off[i] (n offsets; the arena carries 16 bytes of slack behind the last record).  The
 * dictionary is the host's: ref_len (n_ref entries) and ref_names, the n_ref names one after the other, each
 * NUL-terminated, names_bytes bytes in all (as oge_ctx_last_refs hands them out; read only with
 * OGE_TARGETS_TEXT).  *d_targets (device, result->targets entries) and *d_text (device, result->text_bytes
 * bytes; d_text may be NULL without OGE_TARGETS_TEXT) are valid until the next call on ctx; NULL when empty. */
int oge_targets_dev(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, int32_t n_ref,
                    const int32_t *ref_len, const char *ref_names, uint64_t names_bytes, const oge_targets_opts *opts,
                    oge_targets_result *result, const oge_target **d_targets, const uint8_t **d_text);
/* Host-buffer form: uploads, computes, copies the records into targets_out (targets_cap entries) and the text into
 * text_out (text_cap bytes); OGE_ERR_LIMIT with *result filled when either is too small, so a first call with
 * both caps 0 sizes the buffers. */
int oge_targets(oge_ctx *ctx, const uint8_t *recs, uint64_t rec_bytes, const uint64_t *rec_off, uint64_t n, int32_t n_ref,
                const int32_t *ref_len, const char *ref_names, uint64_t names_bytes, const oge_targets_opts *opts,
                oge_targets_result *result, oge_target *targets_out, uint64_t targets_cap, uint8_t *text_out,
                uint64_t text_cap);
/* A whole BAM file resident in HBM (4-byte aligned): framing index, inflate, header, record walk, then the
 * targets against the file's own reference list (which stays with the context for oge_ctx_last_refs). */
int oge_bam_targets_dev(oge_ctx *ctx, const uint8_t *d_z, uint64_t zbytes, const oge_targets_opts *opts,
                        oge_targets_result *result, const oge_target **d_targets, const uint8_t **d_text);

/* ---- NM and MD tags of records in HBM (openge calmd, localrealign --calmd) -------------------------------------
 * The edit distance (NM) and the mismatch string (MD) of every mapped record recomputed against the reference
 * sequence, as `samtools calmd` does without its options (the reference has no such step: it removes MD from every
 * read it moves, algorithms/local_realignment.cpp:881); DESIGN.md section 28, the model is tests/calmd_model.py.
 * Reference: the FASTA at fasta_path through the realigner's loader (name up to the first blank, CR before LF
 *   dropped, the last of a repeated name wins), a..z upper-cased; only the contigs the list names are kept.
 * Passed through unchanged, byte for byte, and counted in `skipped`: FLAG 0x4 set; refID < 0 or pos < 0;
 *   n_cigar_op == 0; l_seq == 0.  A record of a contig whose name the FASTA lacks is passed through too and counted
 *   in `no_reference`.  Every other record is used.
 * Walk of a used record: x = pos (reference), y = 0 (read), run u = 0, nm = 0, MD empty; the ops in order.
 *   M, =, X  per base: x at or past the end of the loaded sequence ends the walk of this record there, for all later
 *            ops too (MD closes with the current run).  Otherwise c1 = the read's 4-bit code, c2 = the code of the
 *            reference byte in "=ACMGRSVTWYHKDBN" (any other byte: 15); c1 == 0, or c1 == c2 and c1 != 15, is a
 *            match (u += 1); anything else appends decimal u and the reference byte, u = 0, nm += 1 (N against N is
 *            a mismatch, as in samtools).
 *   D of L   appends decimal u, '^' and the L reference bytes from x, cut at the end of the sequence; u = 0,
 *            nm += L, x += L.       I: y += L, nm += L.     S: y += L.     N: x += L.     H, P: nothing.
 *   At the end decimal u is appended (it may be "0").
 * Tags: every tag is walked (A c C: 1 byte, s S: 2, i I f: 4, Z H: up to the NUL, B: subtype, count, elements) and
 *   only the first tag named NM and the first named MD are looked at.  NM of an integer type (c C s S i I) whose
 *   value equals nm stays where and as it is; otherwise an NM tag of whatever type is removed and a new one
 *   appended at the record's end with the smallest unsigned type that holds nm (C, S, I).  MD of type Z whose bytes
 *   equal the new string stays; otherwise it is removed and MD:Z appended, after the NM tag when one was appended.
 *   Every other tag (UQ too) is copied unchanged, block_size is updated, no other core field changes (bin neither).
 * Result: records (= n), skipped, no_reference, nm_changed and md_changed (a tag that was absent and is appended
 *   counts), bytes_out.
 * OGE_ERR_ARG (the message names the lowest such record): a used record with refID >= n_ref (checked before the
 *   FASTA is asked for the contig), a block_size above OGE_MAX_BLOCK_SIZE (10000, what the readers admit), a CIGAR
 *   that does not fit its block_size, a CIGAR op code above 8, bases,
 *   qualities or tags that do not fit block_size (a tag cut by the record's end, an unknown type or B subtype, a
 *   string without its NUL), or M I S = X op lengths that do not sum to l_seq; unknown option bits, no FASTA path,
 *   names that are not n_ref NUL-terminated strings.  OGE_ERR_LIMIT, likewise named: a record whose block_size
 *   would exceed OGE_MAX_BLOCK_SIZE (10000) after the update, or whose nm exceeds 2^32 - 1.  OGE_ERR_IO: the FASTA
 *   cannot be read or holds no sequence.  Nothing is written for a call that fails.
 * The FASTA is an argument of every call, not a call of its own: the context keeps the uploaded sequences and
 *   uploads again only when the file's path, size or mtime or the contig list differ from the last call's, so a
 *   caller has no load to order before its calls and none to repeat when the file changes.  Counter
 *   (oge_ctx_counter) "calmd_ref_uploads" = the uploads of the context's lifetime up to and including this call.
 * Stage name for oge_ctx_timing: "calmd"; nested in it "calmd_ref", "calmd_size" (with the scan), "calmd_emit". */
typedef struct oge_calmd_opts {
    int32_t threads; /* host threads that read and lay out the FASTA; 0: one per hardware thread */
    uint32_t flags;  /* 0 */
} oge_calmd_opts;
void oge_calmd_opts_init(oge_calmd_opts *o);
typedef struct oge_calmd_result {
    uint64_t records, skipped, no_reference, nm_changed, md_changed, bytes_out;
} oge_calmd_result;
/* Records d_recs + d_off[i] (n offsets; the arena carries 16 bytes of slack behind the last record).  The contig
 * list is the host's: the n_ref names one after the other, each NUL-terminated, names_bytes bytes in all (as
 * oge_ctx_last_refs hands them out).  *d_out (device, result->bytes_out bytes and 16 of slack) and *d_out_off
 * (device, n + 1 offsets from 0) belong to the context and are valid until the next call on it. */
int oge_calmd_dev(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, int32_t n_ref, const char *ref_names,
                  uint64_t names_bytes, const char *fasta_path, const oge_calmd_opts *opts, oge_calmd_result *result,
                  const uint8_t **d_out, const uint64_t **d_out_off);
/* Host-buffer form: uploads, computes, copies the records into recs_out (out_cap bytes) and their n + 1 offsets
 * into off_out; OGE_ERR_LIMIT with *result filled when recs_out is too small, so a first call with out_cap 0 sizes
 * the buffer. */
int oge_calmd(oge_ctx *ctx, const uint8_t *recs, uint64_t rec_bytes, const uint64_t *rec_off, uint64_t n, int32_t n_ref,
              const char *ref_names, uint64_t names_bytes, const char *fasta_path, const oge_calmd_opts *opts,
              oge_calmd_result *result, uint8_t *recs_out, uint64_t out_cap, uint64_t *off_out);
/* A whole BAM file resident in HBM (4-byte aligned): framing index, inflate, header, record walk, then the tags
 * against the file's own reference list (which stays with the context for oge_ctx_last_refs). */
int oge_bam_calmd_dev(oge_ctx *ctx, const uint8_t *d_z, uint64_t zbytes, const char *fasta_path, const oge_calmd_opts *opts,
                      oge_calmd_result *result, const uint8_t **d_out, const uint64_t **d_out_off);

/* ---- duplication metrics of marked records (dedup --metrics, mergesort -M --metrics, openge dupmetrics) ----
 * Picard MarkDuplicates' metrics file for records that already carry their final FLAG (the reference writes none,
 * algorithms/mark_duplicates.cpp); DESIGN.md section 26, the model is tests/dupmetrics_model.py.  The counts are
 * a pure function of the marked records: each contributes its FLAG, its refID and the library of its RG tag.
 * Library of a record: the RG value as the dedup's input pass finds it (FindTag semantics: the tags walked from
 *   the end of QUAL; the first tag named RG, of whatever type byte, gives the bytes up to the next NUL or the
 *   record's end; the walk ends without one at a type byte of 0, an unknown type, a B array whose header does not
 *   fit, whose subtype is unknown or whose count is negative, and when the next tag would start at or past the
 *   record's end or with a NUL; a block_size outside [32, 10000] has no tags to walk).  A non-empty value found in
 *   rg_ids of oge_markdup_opts gives rg_lib[g] (the first such g); no tag, an empty or an unlisted value gives
 *   unknown_lib.  EVERY record is resolved, unmapped and secondary ones too.
 * Class of a record, the first rule that applies (buildSortedReadEndLists, :202-209): FLAG 0x4 set or refID == -1:
 *   unmapped; 0x100 set: secondary; 0x1 set and 0x8 clear: pair; otherwise unpaired.  0x800 has no meaning of its own.
 * Counters, all counts of READS, so that the counts of any partition of a record set add up: the four classes, and
 *   unpaired_dups / pair_read_dups = the records of class unpaired / pair whose FLAG has 0x400 (a secondary or
 *   unmapped record with 0x400 counts only under its class).
 * Derived (oge_dup_metrics_text): READ_PAIRS_EXAMINED = pair_reads_examined / 2 and READ_PAIR_DUPLICATES =
 *   pair_read_dups / 2, both floored; READ_PAIR_OPTICAL_DUPLICATES = 0; PERCENT_DUPLICATION = (unpaired_dups +
 *   pair_read_dups) / (unpaired_examined + pair_reads_examined), 0 when the denominator is 0;
 *   ESTIMATED_LIBRARY_SIZE by oge_estimate_library_size(READ_PAIRS_EXAMINED, READ_PAIRS_EXAMINED -
 *   READ_PAIR_DUPLICATES); the ROI histogram at x = 1..100 is L * (1 - exp(-(x * n) / L)) / c in double (L the
 *   estimate, n the pairs, c the unique pairs), written only when the file has exactly one row and that row has an
 *   estimate above 0 (with no unique pair the bisection runs on NaNs and leaves 0).
 * Counters (oge_ctx_counter): "dupmetrics_tile_records" = the records one workgroup takes per tile,
 * "dupmetrics_lds_libs" = the libraries whose counts a workgroup sums in LDS (more: the per-wave sums go straight
 * to the table in HBM).  Stage name for oge_ctx_timing: "dup_metrics".
 * The counters' struct has no typedef: its tag is also the name of the host-buffer entry point. */
struct oge_dup_metrics {
    uint64_t unpaired_examined, pair_reads_examined, secondary, unmapped, unpaired_dups, pair_read_dups;
};
/* Records d_recs + d_off[i] (n offsets; the arena carries 16 bytes of slack behind the last record).  Of opts only
 * the read-group table is read (rg_ids, rg_ids_bytes, rg_lib, n_rg, unknown_lib).  out[n_lib], indexed by library
 * id, is SET (callers sum over ranges and ranks); n_lib = 1 + the largest of rg_lib[] and unknown_lib.  Synchronous
 * on the context's stream.  OGE_ERR_ARG: a library id outside [0, n_lib), n_lib outside [1, 32768]. */
int oge_dup_metrics_dev(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, const oge_markdup_opts *opts,
                        int32_t n_lib, struct oge_dup_metrics *out);
/* Host-buffer form: uploads the records and offsets, then the same. */
int oge_dup_metrics(oge_ctx *ctx, const uint8_t *recs, uint64_t rec_bytes, const uint64_t *rec_off, uint64_t n,
                    const oge_markdup_opts *opts, int32_t n_lib, struct oge_dup_metrics *out);
/* A whole BAM file resident in HBM (4-byte aligned): framing index, inflate, header, record walk, then the counts
 * against the read-group table of the file's own header, numbered as oge_bam_markdup_opts numbers it.  *out
 * (*n_lib entries, by library id) and *lib_names (the *n_lib names NUL-terminated one after the other, names_bytes
 * in all; "" for an id that no @RG names) are host memory of the context, valid until its next call of this
 * function.  *unknown_lib = the id of "Unknown Library": that of the @RG lines without an LB, or an id of its own,
 * then without a name, when every @RG has one. */
int oge_bam_dup_metrics_dev(oge_ctx *ctx, const uint8_t *d_z, uint64_t zbytes, const struct oge_dup_metrics **out, int32_t *n_lib,
                            const char **lib_names, uint64_t *names_bytes, int32_t *unknown_lib);
/* Picard's estimateLibrarySize, host only, all in double in this order of operations: n = pairs, c = unique_pairs,
 * f(x) = c / x - 1 + exp(-n / x); no estimate (returns 1, *size untouched) unless n > 0 and n - c > 0; m = 1,
 * M = 100; while f(M * c) > 0: M *= 10; 40 bisection steps on r = (m + M) / 2 with u = f(r * c): stop at u == 0,
 * m = r when u > 0, else M = r; *size = (uint64)(c * (m + M) / 2), returns 0. */
int oge_estimate_library_size(uint64_t pairs, uint64_t unique_pairs, uint64_t *size);
/* The metrics file, host only.  n_rows rows: names[i] (NUL-terminated) with the counters m[i], written sorted by
 * name in byte order; command_line goes behind "# " on the second line.
 *   ## htsjdk.samtools.metrics.StringHeader / # <command line> / <blank> /
 *   ## METRICS CLASS<TAB>picard.sam.DuplicationMetrics / the ten column names / one row per library / <blank> /
 *   [## HISTOGRAM<TAB>java.lang.Double / BIN<TAB>VALUE / 100 lines "x.0<TAB>%.6f" / <blank>]
 * Integers in decimal, PERCENT_DUPLICATION as %.6f, the library size empty when there is no estimate.
 * *len_out = the bytes of the whole text; buf (cap bytes, may be NULL with cap 0) gets min(cap - 1, *len_out)
 * of them and a NUL, as oge_bam_header_text does. */
int oge_dup_metrics_text(const char *const *names, const struct oge_dup_metrics *m, int32_t n_rows, const char *command_line, char *buf,
                         uint64_t cap, uint64_t *len_out);

/* ---- duplicate sets: optical duplicates and set-size histograms (--optical-distance N) ------------------------
 * What the six counters above cannot give: the pair duplicate SETS of records resident in HBM, per library their
 * optical duplicates, over all libraries three set-size histograms.  DESIGN.md section 27; the model is
 * tests/dupsets_model.py.  Picard is not part of the tests: no byte parity with it is claimed.
 * Pairs and sets are exactly the dedup's: ReadEnds of mapped primary records, the ends of one RG:name paired up
 *   consecutively in record order, a set = the pairs with equal (library, read-1 refID, read-1 5' coordinate,
 *   orientation, read-2 refID, read-2 5' coordinate); a set of one pair is a set.  The duplicate flags are not
 *   read: a marked and an unmarked file give the same result, in any record order that keeps each name's ends in
 *   their relative order.
 * Location of a pair, from the name of its read 1 (the leftmost end; the bytes before the NUL): split at ':'; with
 *   exactly 5 or exactly 7 fields the last three are tile, x, y; any other count: no location.  A number is an
 *   optional '-', then decimal digits up to the first other byte (trailing bytes are ignored, no digit gives 0),
 *   held in int32 (the result of more than 9 digits is not defined).  The tile is kept as int32 (Picard narrows it
 *   to 16 bits: a stated departure).  The read group is the index g the RG walk above resolves read 1's value to
 *   (the first @RG of that id), or -1.
 * Optical duplicates of a set: a set whose orientation is FR or RF (the two ends on different strands) is first
 *   divided in two by whether read 1 has FLAG 0x40; FF and RR sets are not divided.  Within a part two located
 *   pairs are close when they have the same read-group index and tile, |dx| <= D and |dy| <= D; the part
 *   contributes (located members) - (connected components of "close"); the sum over the parts goes to the set's
 *   library.
 * Histograms: OGE_DUP_SETS_BINS u64 bins per column, a value counted at min(value, bins - 1), all libraries
 *   together, every set counted: for a set of s pairs with o optical duplicates all_sets[s]++,
 *   non_optical_sets[s - o]++, and optical_sets[o + 1]++ when o > 0.  hist holds the three columns one after the
 *   other in that order of the text: all_sets, optical_sets, non_optical_sets.
 * Per library: pairs, sets, optical, and located = the pairs with a location in sets of two or more pairs (the
 *   only ones whose names are read).  pairs - sets equals READ_PAIR_DUPLICATES of the marked records unless a
 *   candidate end has a mate refID of -1.
 * The pass repeats the dedup's ReadEnds pass and mate join (no kernel of theirs is changed), groups the pairs
 * exactly (two stable radix sorts on the varying key bits, head flags, a scan), reads the names of the members of
 * sets of two or more, and counts components in three tiers: sets of at most "dupsets_wave_cap" (64) members in a
 * wave, whole sets only; larger ones up to "dupsets_block_cap" in one workgroup's LDS; larger ones by an exact
 * union-find on the host ("dupsets_host_sets").  Counters "dupsets_wave_sets" and "dupsets_block_sets" count the
 * sets of two or more pairs the first two tiers took.  Stage "dup_sets", with sub-stages "ds_readends", "ds_join",
 * "ds_group", "ds_locate", "ds_components".
 * OGE_ERR_LIMIT: n >= 2^31, n_lib > 2048.  OGE_ERR_ARG: distance < 0, a library id outside [0, n_lib). */
#define OGE_DUP_SETS_BINS 1024
struct oge_dup_sets_lib {
    uint64_t pairs, sets, located, optical;
};
/* Records as for oge_dup_metrics_dev; opts as for oge_markdup_dev (the read-group table and n_ref; split_chains
 * must be <= 1 and compat_nonverbose_index 0).  out_per_lib[n_lib] and hist[3 * OGE_DUP_SETS_BINS] are SET.
 * Synchronous on the context's stream. */
int oge_dup_sets_dev(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, const oge_markdup_opts *opts,
                     int64_t distance, int32_t n_lib, struct oge_dup_sets_lib *out_per_lib, uint64_t *hist);
/* Host-buffer form: uploads the records and offsets, then the same. */
int oge_dup_sets(oge_ctx *ctx, const uint8_t *recs, uint64_t rec_bytes, const uint64_t *rec_off, uint64_t n,
                 const oge_markdup_opts *opts, int64_t distance, int32_t n_lib, struct oge_dup_sets_lib *out_per_lib, uint64_t *hist);
/* A whole BAM file resident in HBM, as oge_bam_dup_metrics_dev: the libraries numbered from the file's own header.
 * *out_per_lib (*n_lib entries) and *hist (3 * OGE_DUP_SETS_BINS) are host memory of the context, valid until its
 * next call of this function. */
int oge_bam_dup_sets_dev(oge_ctx *ctx, const uint8_t *d_z, uint64_t zbytes, int64_t distance, const struct oge_dup_sets_lib **out_per_lib,
                         const uint64_t **hist, int32_t *n_lib);
/* The metrics file with the optical column filled and the set-size histogram, host only.  Rows as for
 * oge_dup_metrics_text, s[i] beside m[i]: READ_PAIR_OPTICAL_DUPLICATES = s[i].optical, ESTIMATED_LIBRARY_SIZE =
 * oge_estimate_library_size(READ_PAIRS_EXAMINED - optical, READ_PAIRS_EXAMINED - READ_PAIR_DUPLICATES) (none when
 * optical or the duplicates exceed the pairs), the ROI from the same two arguments.  The histogram block is always
 * written: "## HISTOGRAM<TAB>java.lang.Double", the column line BIN, then CoverageMult only with exactly one row
 * that has an estimate above 0, then all_sets, optical_sets, non_optical_sets; one line per BIN from 1 to the
 * largest non-empty bin of the three columns (to 100 if the ROI column is there and that is larger; past 100 the
 * ROI continues by the same formula); BIN as "%d.0", the ROI as %.6f, the counts as integers; a blank line. */
int oge_dup_sets_text(const char *const *names, const struct oge_dup_metrics *m, const struct oge_dup_sets_lib *s, int32_t n_rows,
                      const uint64_t *hist, const char *command_line, char *buf, uint64_t cap, uint64_t *len_out);

/* ---- SAM and FASTQ text of records in HBM (openge view, -F sam|fastq) ----------------------------------
 * The reference's SamWriter::write (util/sam_writer.cpp:90-217) and the single-stream form of
 * FastqWriter::write (util/fastq_writer.cpp:99-100) on the device; DESIGN.md section 21.
 * SAM line: QNAME FLAG RNAME POS+1 MAPQ CIGAR, the mate fields, SEQ, QUAL, the tags, tab separated, "\n".
 * RNAME is "*" when refID is outside [0, n_ref); CIGAR "*" without ops (letters MIDNSHP=X, '?' for codes 9-15);
 * the mate fields are ("=" | the mate's contig) MPOS+1 TLEN when FLAG 0x1 is set and 0 <= mate refID < n_ref,
 * else "*" 0 0; SEQ from the 4-bit codes by "=ACMGRSVTWYHKDBN" and QUAL as byte + 33 (wrapping at 8 bits), both
 * "*" when l_seq is 0; tags A, c C s S i I (all printed i:), Z and H in record order; a NUL byte behind a tag's
 * value ends the tag list (sam_writer.cpp:210).  POS+1 and MPOS+1 are computed in 64 bits.
 * FASTQ entry: "@" name "\n" SEQ "\n+" name "\n" QUAL "\n" with SEQ and QUAL cut to [trim_begin,
 * l_seq - trim_end) (Filter::trim, algorithms/filter.cpp:183-190; empty when l_seq <= trim_begin + trim_end).
 * SEQ under a trim window is the reference's; its QUAL is not reproduced: Filter::trim cuts the qualities of
 * the read it has already shortened a second time, which leaves fewer qualities than bases, bytes from behind
 * the qualities in reads without tags, and an abort on short reads.
 * Records with an f or a B tag are formatted on the host (f as printf "%g", B as the SAM specification's
 * XX:B:t,v,v with %g float elements; the reference's switch has no B case): the device marks them, gives
 * them length 0 and leaves them out.  A record with any other tag type, with a tag or a Z string cut short,
 * or whose lengths do not fit its block_size fails the size call with OGE_ERR_ARG naming the record index. */
enum { OGE_TEXT_SAM = 0, OGE_TEXT_FASTQ = 1 };
typedef struct oge_text_opts {
    int32_t mode;                 /* OGE_TEXT_SAM / OGE_TEXT_FASTQ */
    int32_t trim_begin, trim_end; /* FASTQ only, >= 0 */
    int32_t n_ref;
    const char *ref_names;        /* host: the n_ref contig names back to back, no separators */
    const uint32_t *ref_name_off; /* host: n_ref + 1 offsets into ref_names */
} oge_text_opts;
/* Size pass and scan.  Records d_recs + d_off[i] (n offsets read; the arena carries 16 bytes of slack behind
 * the last record).  d_text_off (n + 1 entries): the exclusive scan of the text lengths, 0 for marked records;
 * d_host_mark (n bytes): 1 for a record the host formats, else 0.  *total = d_text_off[n], *n_host = the
 * marked records, also the context counter "sam_host_lines".  The contig table is uploaded when it differs
 * from the last call's.  OGE_ERR_LIMIT when n >= 2^32 - 1.  Stage name for oge_ctx_timing: "text_size". */
int oge_text_size_dev(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, const oge_text_opts *opts,
                      uint64_t *d_text_off, uint8_t *d_host_mark, uint64_t *total, uint64_t *n_host);
/* Emit pass: the text of records [first, first + count) at d_out + d_text_off[i] - d_text_off[first]; cap >=
 * d_text_off[first + count] - d_text_off[first] (OGE_ERR_LIMIT otherwise, nothing is written).  opts and
 * d_text_off as in the size call that filled d_text_off.  Counters "text_wave_records" / "text_block_records":
 * the records one wave / one workgroup of the kernel takes.  Stage name: "text_emit". */
int oge_text_emit_dev(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, const uint64_t *d_text_off, uint64_t first,
                      uint64_t count, const oge_text_opts *opts, uint8_t *d_out, uint64_t cap);
/* One record's text on the host, every tag type included (the lines the device leaves out): written to buf
 * when cap holds it, *len = its length (OGE_ERR_LIMIT when cap is smaller, with *len set).  rec_bytes =
 * block_size + 4. */
int oge_text_host_line(const uint8_t *rec, uint64_t rec_bytes, const oge_text_opts *opts, char *buf, uint64_t cap, uint64_t *len);
/* Host-buffer form: uploads, sizes, emits, downloads and splices the host-formatted lines in at their places.
 * *bytes = the whole text's length; OGE_ERR_LIMIT when cap is smaller (with *bytes set, nothing written). */
int oge_text_format(oge_ctx *ctx, const uint8_t *recs, uint64_t rec_bytes, const uint64_t *rec_off, uint64_t n,
                    const oge_text_opts *opts, uint8_t *out, uint64_t cap, uint64_t *bytes);

/* ---- SAM text in HBM -> BAM records in HBM (SAM input of every command) ---------------------------------
 * The reference's SamReader::ParseAlignment (util/sam_reader.cpp:313-488) on the device, the inverse of the
 * text calls above; DESIGN.md section 22.  A line is QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ QUAL
 * and any number of tags XX:T:value, tab separated.  The record stores POS - 1 and PNEXT - 1, TLEN as it is,
 * bin from POS - 1 and the CIGAR's reference length (CalculateMinimumBin, util/bam_serializer.h:92-116: POS 0
 * without CIGAR gives 4680); RNAME and RNEXT become refIDs through the contig table of opts (only n_ref,
 * ref_names and ref_name_off of oge_text_opts are read; of two contigs with one name the first is found): "*"
 * is -1, "=" as RNEXT the read's own refID, an RNEXT the table does not have is -1 and sets the line's warning
 * byte (the reference prints "RNext X missing from sequence dictionary"), an RNAME it does not have is an error
 * whose message begins with the reference's "Rname X missing from sequence dictionary".  CIGAR "*" gives no
 * ops, otherwise <length below 2^28><one of MIDNSHP=X> up to 65535 times.  SEQ is packed by "=ACMGRSVTWYHKDBN"
 * in either case (any other character is N), "*" is l_seq 0; QUAL is byte - 33, "*" is l_seq bytes of 0xFF.
 * Tags: A; i in the reference's smallest type (C for 0..255, c for -128..-1, S up to 65535, s down to -32768,
 * then I up to 2^32-1, then i); Z and H as their strings; f (strtof) and B:t,v,... (the specification's array)
 * only on the host: the size pass gives their lines the exact length and marks them, the emit pass stores
 * every other byte of such a record, and the caller copies oge_sam_host_record's record over it.
 * Everything else is an error (OGE_ERR_ARG, the message names the 1-based line of the file and the field):
 * fewer than 11 fields, a line shorter than 10 characters, a number that is not -?[0-9]+ or outside its
 * field's range (FLAG 0..65535, MAPQ 0..255, POS - 1 and PNEXT - 1 and TLEN in 32 bits, a tag integer in
 * -2^31..2^32-1), QNAME longer than 254 characters, QUAL of another length than SEQ, a tag not shaped XX:T:,
 * a type outside AifZHB, more than 65535 CIGAR ops, a line of more than 2^30 characters.  A '\r' is a
 * character like any other.  The text needs no slack behind its last byte. */
/* The length of the leading lines that begin with '@' (the header) and their count (may be NULL). */
int oge_sam_header(const char *text, uint64_t bytes, uint64_t *header_len, uint64_t *header_lines);
/* Line index of d_text[body_off, bytes) (d_text 4-byte aligned): *n = the lines (a last line without "\n"
 * is a line, a trailing "\n" adds none).  With d_line_off NULL it only counts; else d_line_off (cap >= n + 1
 * entries, OGE_ERR_LIMIT otherwise) gets d_line_off[0] = body_off and d_line_off[i + 1] = one past the
 * position of line i's newline (bytes + 1 for a last line without one), so line i is d_text[d_line_off[i],
 * d_line_off[i + 1] - 1).  OGE_ERR_LIMIT when n >= 2^32 - 1.  Stage name for oge_ctx_timing: "sam_lines". */
int oge_sam_lines_dev(oge_ctx *ctx, const uint8_t *d_text, uint64_t bytes, uint64_t body_off, uint64_t *d_line_off, uint64_t cap,
                      uint64_t *n);
/* Size pass and scan.  d_rec_off (n + 1 entries): the exclusive scan of the exact record lengths (block_size
 * field included), host-marked lines included, so the arena has no holes; d_host_mark (n bytes): 1 for a line
 * with an f or B tag; d_warn (n bytes): 1 for a line whose RNEXT the table does not have.  *total =
 * d_rec_off[n], *n_host = the marked lines, also the context counter "sam_host_lines"; counters
 * "sam_wave_lines" / "sam_block_lines": the lines one wave / one workgroup of the kernels takes.  On a bad line
 * OGE_ERR_ARG: the message names the lowest bad line (1-based in the file: the lines of d_text[0, d_line_off[0])
 * count) and its field, counters "sam_bad_line" and "sam_bad_code"; d_rec_off, d_host_mark and d_warn are then left
 * as they were.  The contig
 * table is uploaded when it differs from the last call's (counter "sam_table_uploads").  Stage name: "sam_size". */
int oge_sam_size_dev(oge_ctx *ctx, const uint8_t *d_text, const uint64_t *d_line_off, uint64_t n, const oge_text_opts *opts,
                     uint64_t *d_rec_off, uint8_t *d_host_mark, uint8_t *d_warn, uint64_t *total, uint64_t *n_host);
/* Emit pass: the records of lines [first, first + count) at d_recs + d_rec_off[i] - d_rec_off[first]; cap >=
 * d_rec_off[first + count] - d_rec_off[first] (OGE_ERR_LIMIT otherwise, nothing is written).  opts as in the
 * size call that filled d_rec_off.  Nothing is stored outside a record's own bytes.  Stage name: "sam_emit". */
int oge_sam_emit_dev(oge_ctx *ctx, const uint8_t *d_text, const uint64_t *d_line_off, const uint64_t *d_rec_off, uint64_t first,
                     uint64_t count, const oge_text_opts *opts, uint8_t *d_recs, uint64_t cap);
/* One line's record (line[0, len), no newline) on the host, every tag type included: written to buf when cap
 * holds it, *len_out = its length (OGE_ERR_LIMIT when cap is smaller, with *len_out set).  OGE_ERR_ARG with
 * the field's name for a line that does not parse. */
int oge_sam_host_record(const char *line, uint64_t len, const oge_text_opts *opts, uint8_t *buf, uint64_t cap, uint64_t *len_out);
/* Host-buffer form: splits the header (*header_len = the bytes of the leading '@' lines), builds the contig
 * table from its @SQ lines as the header model reads them (oge_bam_header_text's parser; a header it refuses
 * is OGE_ERR_ARG), uploads, indexes, sizes, emits, builds the marked lines' records on the host and downloads.  *recs (*rec_bytes bytes and 16 bytes of slack), *rec_off (*n + 1 entries) and *warn
 * (*n bytes, may be NULL) are the context's, valid until its next oge_sam_parse call.  On an error nothing is
 * handed back (the pointers are NULL, *n is 0). */
int oge_sam_parse(oge_ctx *ctx, const char *text, uint64_t bytes, uint64_t *header_len, const uint8_t **recs, uint64_t *rec_bytes,
                  const uint64_t **rec_off, uint64_t *n, const uint8_t **warn);

/* ---- mergesort extras: Filter (-r region / -q mapq) and sort by name (-b) ----------- */
/* Filter::runInternal's predicate (algorithms/filter.cpp:205-249) with the module's setters
 * (filter.h:34-47).  len = l_seq (BamAlignment::getLength).  A record is kept when
 *   mapq >= mapq_min && min_len <= len <= max_len && len > trim_total
 *   [&& ref_id <= refID <= ref_id && pos + len >= left_pos && pos <= right_pos   if has_region]
 * and at most count_limit records (the first ones kept, in input order) are kept. */
typedef struct oge_filter_opts {
    int32_t has_region;
    int32_t ref_id;       /* region refID (Filter::ParseRegionString) */
    int32_t left_pos;     /* region start, 0-based as the reference compares it */
    int32_t right_pos;    /* region stop */
    int32_t mapq_min;     /* setQualityLimit, default 0 */
    int32_t min_len;      /* setMinimumReadLength, default 0 */
    int32_t max_len;      /* setMaximumReadLength, default INT32_MAX */
    int32_t trim_total;   /* trim_begin_length + trim_end_length, default 0 */
    uint64_t count_limit; /* setCountLimit, default INT32_MAX */
} oge_filter_opts;
/* Defaults of Filter::Filter() (filter.cpp:185-194). */
void oge_filter_opts_init(oge_filter_opts *o);
/* Filter::ParseRegionString (filter.cpp:31-137): "chr", "chr:pos" or "chr:start..stop" against the
 * header's sequence dictionary (ref_names = n_ref NUL-terminated names back to back, ref_len =
 * their LN).  Fills has_region/ref_id/left_pos/right_pos; OGE_ERR_ARG with the reference's message
 * (oge_last_error(NULL)) when the region does not parse or lies outside the sequence. */
int oge_parse_region(const char *region, const char *ref_names, int32_t n_ref, const int64_t *ref_len,
                     oge_filter_opts *o);
/* Copy the records the filter keeps, in input order, to d_out / d_out_off (*n_out records). */
int oge_filter_records_dev(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n,
                           const oge_filter_opts *o, uint8_t *d_out, uint64_t *d_out_off, uint64_t *n_out);
/* One region of a region list (view / mergesort -L): the ref_id, left_pos and right_pos of oge_filter_opts. */
typedef struct oge_region {
    int32_t ref_id, left_pos, right_pos;
} oge_region;
/* The same compaction against a list of regions (a host array, n_regions >= 1; OGE_ERR_ARG otherwise): a
 * record is kept when the predicate above holds without its region part and
 *   refID == ref_id && pos + len >= left_pos && pos <= right_pos
 * holds for AT LEAST ONE region; every kept record is written once, in input order, at most count_limit of
 * them.  has_region and the region fields of `o` are not read.  The regions are sorted by (ref_id, left_pos)
 * on the device and given the running maximum of right_pos within their ref_id; a record then needs one
 * binary search (the last region with left_pos <= pos + len) and one compare (that maximum >= pos), whatever
 * n_regions is and however the regions overlap.  With one region the output equals oge_filter_records_dev's
 * byte for byte.  All scratch sized by n_regions is released before the call returns.  Stage names for
 * oge_ctx_timing: "filter_regions" (sort and maxima), "filter" (the predicate). */
int oge_filter_regions_dev(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n,
                           const oge_filter_opts *o, const oge_region *regions, uint64_t n_regions, uint8_t *d_out,
                           uint64_t *d_out_off, uint64_t *n_out);
/* Sort::ByName (util/bamtools/Sort.h:67-90) as ReadSorter uses it for SORT_QUERYNAME
 * (algorithms/read_sorter.cpp:202-203): read names compared bytewise (std::string <); records
 * with equal names keep input order (the reference's std::sort leaves their order
 * implementation-defined).  d_perm (n) receives the input index of each output position. */
int oge_sort_name_dev(oge_ctx *ctx, const uint8_t *d_recs, const uint64_t *d_off, uint64_t n, uint32_t *d_perm);
int oge_sort_name(oge_ctx *ctx, const uint8_t *recs, uint64_t rec_bytes, const uint64_t *rec_off, uint64_t n,
                  uint32_t *perm_out);

#ifdef __cplusplus
}
#endif
#endif /* OPENGE_HIP_H */
