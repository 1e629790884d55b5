/*
 * kmx.h -- C ABI of the MI355X-native kmtricks counting/merge engine (libkmx.so).
 *
 * This is the drop-in boundary: the entry points below are what the
 * reference's tasks would bind instead of running their CPU classes
 * (file:line relative to the kmtricks source tree):
 *
 *   kmx_merge / kmx_merge_dev   replace km::KmerMerger<MAX_K,MAX_C>::{next,write_as_bin,write_as_pa}
 *                               (include/kmtricks/merge.hpp:102-361) and km::HashMerger<MAX_C>::
 *                               {next,write_as_bin,write_as_pa,write_as_bf,write_as_bfc}
 *                               (merge.hpp:363-629), called from KmerMergeTask::exec / HashMergeTask::exec
 *                               (include/kmtricks/task.hpp:690-743, 787-863)
 *   kmx_count_kmer              replaces km::KmerPartCounter::execute + KmerCountProcessor::process
 *                               (include/kmtricks/gatb/sorting_count.hpp:637-884,
 *                                include/kmtricks/gatb/count_processor.hpp:135-146), CountTask::exec (task.hpp:367-392)
 *   kmx_count_hash              replaces km::HashPartCounter::execute + HashCountProcessor::process
 *                               (sorting_count.hpp:346-363, 908-997; count_processor.hpp:61-70),
 *                               HashCountTask::exec (task.hpp:447-481)
 *   kmx_transpose_bits          replaces km::BitMatrix::transpose / __sse_trans
 *                               (include/kmtricks/bitmatrix.hpp:209-214, 238-289); HashMerger::write_as_bft (merge.hpp:631-644)
 *                               as a whole is kmx_merge* with KMX_MODE_BFT (merge + transpose without leaving HBM)
 *   kmx_filter_dev / _host      replace km::FilterTask::{exec,f_count_matrix,f_pa_matrix} on top of km::MatrixFilter
 *                               (include/kmtricks/matrix.hpp:23-393), run by main_filter (include/kmtricks/cmd.hpp:609-724):
 *                               one partition's matrix rows joined with the new sample's count list
 *   kmx_query_dev / _host       no counterpart in the 1.6.0 tree (kmtricks 1.0's `kmtricks query`): query sequences against the .cmbf
 *                               matrices of a hash:bf:bin run, addressed as kmer_hash.hpp:244-328 and repartition.hpp:94-103 publish
 *   kmx_kquery_dev / _host      no counterpart either: query sequences against the .count / .pa k-mer matrices of a kmer:count:bin /
 *                               kmer:pa:bin run -- exact, with abundances (k-mer, minimizer and partition as kmx_query_* has them)
 *   kmx_zquery_dev / _host      no counterpart either: kmx_query_*'s question asked for (k + z)-mers, the findere trick against Bloom
 *                               false positives -- a position counts for a sample when its z + 1 overlapping k-mers all do
 *   kmx_cquery_dev / _host      no counterpart either: kmx_query_*'s question asked of the counting Bloom matrices of a hash:bfc:bin run --
 *                               per sample the k-mers at or above an abundance class and the sum of the classes' least counts
 *   kmx_dist_dev / _host        no counterpart either (Simka's question): the sample-by-sample shared k-mer tables of a run's matrices --
 *                               rows that hold both samples, sums of the smaller count -- which the Jaccard and Bray-Curtis distances follow from
 *   kmx_colsums_dev / _host,    no counterpart either (kmdiff's question): the per-sample totals of a run's matrices, and the rows whose
 *   kmx_diff_dev / _host        counts differ between case and control samples by a Poisson likelihood-ratio test, kept in file order
 *   kmx_select_dev / _host      no counterpart either (MUSET's `kmat_tools filter`): a smaller matrix out of a larger one -- a list of
 *                               columns in any order, the rows whose recurrence over them lies in a range, counts or presence/absence
 *   kmx_pan_dev / _host         no counterpart either (pangrowth, Panacus `hist`): how many rows of a matrix 0, 1, ... M of a list of
 *                               samples hold, where each row is first met and first missed along the list, and per sample by recurrence
 *   kmx_colors_dev / _host      no counterpart either (the colour classes of Mantis, Bifrost, Fulgor, GGCAT; the bars of an UpSet plot): the
 *                               distinct sets of samples that occur as a row's presence pattern, the rows of each, every row's class
 *   kmx_gram_dev / _host        no counterpart either (EIGENSTRAT / smartpca; the kinship matrix of a k-mer GWAS): the sample-by-sample
 *                               table of shared rows, each row weighted by its recurrence class -- what the samples' PCs follow from
 *   kmx_assoc_dev / _host       no counterpart either (kmdiff's and EIGENSTRAT's corrected test, a k-mer GWAS): the rows whose presence
 *                               pattern is associated with a phenotype once covariates (the PCs) are projected out, kept in file order
 *   kmx_unitigs_dev / _host     no counterpart either (ggcat behind MUSET's `kmat_tools filter`, kmdiff's merge of its significant k-mers):
 *                               a set of distinct canonical k-mers compacted into the unitigs of its de Bruijn graph
 *   kmx_groupsum_dev / _host    no counterpart either (MUSET's `kmat_tools unitig`): a matrix's rows summed by a label per row -- per
 *                               group and sample the rows present and the counts' sum, the unitig x sample table among others
 *   kmx_kset_dev / _host        no counterpart either: a set of canonical k-mers (duplicates allowed) resident on a device as a hash table
 *                               built for membership at one look-up a base
 *   kmx_match_dev / _host       no counterpart either (kmdiff's map-back, the read fetch of a k-mer GWAS, back_to_sequences): per read the
 *                               k-mers it shares with a kset, their strand, the bases they cover, first and last hit; per k-mer its occurrences
 *   kmx_spectra_dev / _host     no counterpart either (KAT `hist` / `comp`, Merqury's spectra-cn): per sample the rows by count, per pair
 *                               of samples the rows by the two counts -- the tables k-mer completeness and consensus quality follow from
 *   kmx_superk_partition       replaces KmFillPartitions / Sequence2SuperKmer / SuperKmer::save
 *                               (include/kmtricks/gatb/fill_partitions.hpp:59-105, gatb kmer/impl/Sequence2SuperKmer.hpp:80-158,
 *                                gatb kmer/impl/Model.hpp:1086-1139, 1388-1433), SuperKTask::exec (task.hpp:255-320)
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on
 * success or a negative KMX_E_* code, with a message in kmx_last_error().
 * There is NO CPU fallback: without a HIP device kmx_create fails with
 * KMX_E_NODEVICE.  All integers little-endian.  A ctx is used by one host
 * thread at a time (one ctx per pool thread, like the reference's tasks).
 */
#ifndef KMX_H
#define KMX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: kmx_merge_task carries list_on_device (the struct grew: a caller built against version 1 hands tasks of the wrong stride);
 *    kmx_set_file_order.  Callers check kmx_version() == KMX_VERSION before anything else. */
#define KMX_VERSION 2

enum {
  KMX_OK = 0,
  KMX_E_NODEVICE = -1,   /* no HIP device / HIP runtime error at init */
  KMX_E_INVAL    = -2,   /* bad argument */
  KMX_E_NOMEM    = -3,   /* host or device allocation failed */
  KMX_E_HIP      = -4,   /* HIP runtime error during a call */
  KMX_E_UNSUPPORTED = -5,/* configuration outside what this build handles (message says which) */
  KMX_E_INTERNAL = -6    /* a bound inside the library was reached on the device (kmx_colors_*, kmx_unitigs_*: the table's probe bound; kmx_unitigs_*: a cycle walk's); never expected */
};

/* matrix row encodings; names follow kmtricks' --mode <kmer|hash>:<count|pa|bf|bfc>:bin */
enum {
  KMX_MODE_COUNT = 0,  /* row = key + N * u32           (.count / .count_hash body) */
  KMX_MODE_PA    = 1,  /* row = key + ceil(N/8) bytes   (.pa / .pa_hash body)       */
  KMX_MODE_BF    = 2,  /* one ceil(N/8)-byte row per hash of [lower, upper] (.cmbf) */
  KMX_MODE_BFC   = 3,  /* one ceil(N*w/8)-byte row per hash, bitpacker MSB-first    */
  KMX_MODE_BFT   = 4   /* the BF matrix bit-transposed on the device: round_up8(N) rows (row s = sample s) of
                          round_up8(W)/8 bytes -- what HashMerger::write_as_bft dumps (merge.hpp:631-644), and
                          the layout the per-sample Bloom filter files are cut from (howde_utils.hpp:133-187) */
};

typedef struct kmx_ctx kmx_ctx;

int  kmx_version(void);
int  kmx_device_count(void);   /* HIP devices visible to this process (0: none -- libkmx has no CPU fallback) */
/* free and total bytes of a device's memory (hipMemGetInfo) */
int  kmx_device_memory(int device, uint64_t* free_bytes, uint64_t* total_bytes);
/* Round 6.  Takes `bytes` of the device's memory in blocks of 1 GiB, holds them all, and gives them back: on a box whose HBM has not
 * been used since boot the driver clears memory the first time it is handed out (~30 us a MB: 8 ms for a 256 MB store chunk, 18 ms
 * for a 600 MB row arena, with the GPU idle behind the allocating call) and not again afterwards.  `kmx pipeline` calls it on a
 * thread of its own while the first samples are read (KMX_WARM_GB, default 96, 0: never); the count and merge stages' own
 * allocations then find memory that is handed out at once.  Returns the bytes it took (0: nothing to do, or no memory to spare). */
uint64_t kmx_device_warm(int device, uint64_t bytes, const volatile int* stop /* or NULL: checked before every block; non-zero ends the call */);
/* (it times its first block: memory that comes at once -- under 5 ms a GiB -- has been handed out before, and the call returns) */
int  kmx_create(int device, kmx_ctx** out);
void kmx_destroy(kmx_ctx* ctx);
/* last error message of this ctx (or of the failed kmx_create when ctx == NULL) */
const char* kmx_last_error(const kmx_ctx* ctx);
/* When on, the merge driver brackets its dominant kernel with HIP events on the ctx stream so that bench.py can report
 * the kernel's launch duration.  Which kernel a batch runs (libkmx chooses; KMX_MERGE_KERNEL=rows|pivot|cols forces one):
 *   COUNT / PA   k_merge_cols + k_cols_sparse  every task has >= 192 lists (>= 257 for count rows with 64-bit keys in file
 *                                              order, >= 160 / 96 for PA rows with 128-bit keys in file order / not;
 *                                              KMX_COLS_MIN_LISTS[_ORD]), recurrence-min <= 21, share-min <= max(1,
 *                                              recurrence-min), >= 1 M records in the batch; 64- and 128-bit keys
 *                k_merge_pivot                 otherwise, tasks of more than 512 lists, 64-bit keys, no share-min
 *                k_merge_rows                  everything else -- and the tasks the two above hand back (lists that do not
 *                                              resemble each other): results never depend on the choice
 *   BF / BFC     k_merge_bf;   BFT  k_merge_bft */
int  kmx_set_profiling(kmx_ctx* ctx, int on);
/* COUNT / PA rows in FILE ORDER out of the merge itself (default on; KMX_FILE_ORDER=0 in the environment or on = 0 here turns it
 * off).  The reference's output IS the ascending row stream (merge.hpp:262-272 write_as_bin -> io/matrix_file.hpp:120-127).  On:
 * the column-blocked pair writes every row at its final place -- k_cols_sparse learns each slice group's offset by a decoupled
 * look-back and puts the group's rows, the row keys' rows among them, in key order there: the arena IS the matrix body
 * (kmx_result_body_dev returns it, no second copy, no gather pass).  Off: the row keys' rows first, the other rows behind them in
 * runs with a directory (kmx_result_arena + kmx_result_copy_order; kmx_result_body_dev then assembles a copy on the device). */
int  kmx_set_file_order(kmx_ctx* ctx, int on);
/* HIP stream the ctx launches on (a hipStream_t), so callers can order their own work after it */
void* kmx_stream(kmx_ctx* ctx);

/* ------------------------------------------------------------------ merge */

/* One sample's sorted count list of one partition: `n` packed records of
 * key_words*8 key bytes (low word first) + a u32 count = the body of a
 * .kmer count file written with 4-byte counts (io/kmer_file.hpp:102-108).
 * Keys strictly ascending (most significant word first, kmer.hpp:262-268). */
typedef struct {
  const void* recs;
  uint64_t    n;
} kmx_list;

/* One merge task = one partition (merge.hpp:115-125, 376-385). */
typedef struct {
  uint32_t        n_lists;     /* N samples, fof order = column order (kmdir.hpp:65-72).
                                  LIMIT (a deliberate deviation from KmerMerger, which takes any vector of paths, merge.hpp:115-125): a COUNT / PA
                                  task takes at most 4096 lists (3072 with keys of four words) -- a row's cursors and its image live in one
                                  workgroup's LDS; a hash:bft task at most 18396 (the cursors of every sample beside the tile).  Beyond:
                                  KMX_E_UNSUPPORTED, nothing is merged.  BASELINE's largest cohort is 2500.  (BF / BFC windows: no limit of that kind.) */
  uint32_t        key_words;   /* ceil(k / 32) (kmer.hpp:215 m_n_data, io/kmer_file.hpp:84 kmer_slots): 1 for k <= 32 and hash keys, 2 up to 64,
                                  3 up to 96, 4 up to 128.  3 and 4 (the reference's Kmer<96> / Kmer<128>): COUNT / PA rows, at most 4096 (three words) / 3072 (four) lists a task */
  const kmx_list* lists;       /* [n_lists] */
  const uint32_t* soft_min;    /* [n_lists] per-sample abundance min (m_a_min_vec) */
  uint32_t        rec_min;     /* recurrence-min (m_r_min) */
  uint32_t        share_min;   /* share-min / save_if (m_save_if), 0 = no rescue */
  uint32_t        mode;        /* KMX_MODE_* */
  uint32_t        bitw;        /* BFC bits per count (--bitw), else ignored */
  uint64_t        lower, upper;/* BF/BFC: first and last hash of the window (hash.hpp:77-85) */
  uint64_t        rows_hint;   /* COUNT/PA: expected kept rows (0 = let the engine guess) */
  const uint8_t*  list_on_device; /* kmx_merge_host only: NULL = every lists[i].recs is a host pointer; else [n_lists],
                                     non-zero = lists[i].recs is a DEVICE pointer already (a list of a kmx_store) and is
                                     merged where it lies.  Ignored by kmx_merge_dev / kmx_merge. */
} kmx_merge_task;

/* statistics layout: 6 * n_lists u64, rows in the order of merge.hpp:72-83:
 * NON_SOLID, RESCUED, UNIQUE_WO_RESCUE, UNIQUE_W_RESCUE, TOTAL_WO_RESCUE, TOTAL_W_RESCUE */
#define KMX_STATS_ROWS 6

typedef struct kmx_merge_result kmx_merge_result;

/* Device-resident batch merge: every lists[i].recs is a DEVICE pointer (4-byte
 * aligned) whose records are complete, or produced by work queued on kmx_stream(ctx)
 * (libkmx prepares a batch on a second stream of the context; once kmx_stream has been
 * called that stream is ordered behind the first).  Enqueues the whole batch and returns; the
 * result stays in HBM until freed.  COUNT/PA rows are produced in row segments
 * that kmx_result_* hands back in ascending key order. */
int kmx_merge_dev(kmx_ctx* ctx, const kmx_merge_task* tasks, uint32_t n_tasks, kmx_merge_result** out);
/* blocks until the batch has finished on the GPU; returns KMX_OK or the error of the run */
int      kmx_result_wait(kmx_merge_result* r);
/* duration in ms of the batch's merge kernel launch (needs kmx_set_profiling(ctx, 1)); < 0 if unavailable */
double   kmx_result_kernel_ms(kmx_merge_result* r);
/* the same launch in its two kernels when the column-blocked pair produced the result: k_merge_cols (the column blocks' walk over the
 * lists), then k_cols_sparse (the rows of the keys outside the row keys; with kmx_set_file_order on also the row keys' rows at their
 * final place).  -1 in both for every other kernel, without profiling, or when tasks were re-run behind the pair. */
int      kmx_result_kernel_parts_ms(kmx_merge_result* r, double* first_ms, double* second_ms);
/* name of the device kernel that produced (most of) the result: "k_merge_cols", "k_merge_pivot", "k_merge_rows",
 * "k_merge_bf" or "k_merge_bft" (see kmx_set_profiling for when each is chosen); valid after kmx_result_wait (tasks a cohort
 * kernel handed back count for the kernel that completed them) */
const char* kmx_result_kernel(const kmx_merge_result* r);
/* duration in ms of a separate transpose pass behind the merge; < 0 when there is none (KMX_MODE_BFT results come out
 * of k_merge_bft sample-major already: kmx_result_kernel_ms covers k_bf_rowrec + k_merge_bft) */
double   kmx_result_transpose_ms(kmx_merge_result* r);
/* DEVICE pointer to the task's body in file order (rows * row_bytes bytes), valid until kmx_result_free.  BF / BFC / BFT
 * bodies are dense as the kernel leaves them; COUNT / PA rows are put in ascending key order on the device the first time
 * the body is asked for (rows of k_merge_rows / k_merge_pivot lie in arena segments, those of k_merge_cols in two ascending
 * lists): a caller can then bring it to the host in pieces (kmx_copy_to_host) or send it from where it lies. */
const void* kmx_result_body_dev(kmx_merge_result* r, uint32_t task);
/* queues that ordering for a COUNT / PA task without waiting for it (a writer asks for task i + 1 before it brings task i's body
 * over: the pass hides behind the copies); kmx_result_body_dev / kmx_result_copy_body wait for it.  No-op for Bloom results. */
int kmx_result_prepare_body(kmx_merge_result* r, uint32_t task);
uint64_t kmx_result_rows(const kmx_merge_result* r, uint32_t task);        /* kept rows (COUNT/PA), window rows (BF/BFC), round_up8(N) (BFT) */
/* COUNT/PA results of k_merge_cols: how many of the task's rows came out of k_cols_sparse (keys outside the row keys the
 * column blocks are built on: sample-private k-mers, k-mers a few samples share); 0 for the other kernels */
uint64_t kmx_result_sparse_rows(const kmx_merge_result* r, uint32_t task);
uint64_t kmx_result_row_bytes(const kmx_merge_result* r, uint32_t task);
uint64_t kmx_result_body_bytes(const kmx_merge_result* r, uint32_t task);  /* rows * row_bytes */
/* algorithmic bytes moved for this task: input records + output rows (DESIGN.md roofline) */
uint64_t kmx_result_algo_bytes(const kmx_merge_result* r, uint32_t task);
/* copies the matrix file body (rows in ascending key order, exactly what the
 * reference's writer streams after its header) into host memory -- by DMA straight into host_dst when that is
 * page-locked (kmx_alloc_pinned), through a pinned staging buffer otherwise */
int kmx_result_copy_body(kmx_merge_result* r, uint32_t task, void* host_dst, uint64_t dst_bytes);
/* COUNT / PA results WITHOUT any device-side pass over the rows: the arena as the kernels left it (arena_rows rows of row_bytes,
 * some unused) and the order of its rows -- host_order[d] (kmx_result_rows entries) = the arena row that is row d of the body.
 * What a file writer takes: it brings the arena to the host in pieces (kmx_copy_to_host) and writes every run of rows at its
 * place (pwrite at d * row_bytes): the file order comes to exist in the file, never as a second copy of the matrix in HBM. */
int kmx_result_arena(kmx_merge_result* r, uint32_t task, const void** dev_arena, uint64_t* arena_rows);
int kmx_result_copy_order(kmx_merge_result* r, uint32_t task, uint32_t* host_order);
/* the same body into DEVICE memory of the caller (e.g. a buffer an RCCL collective sends from) */
int kmx_result_copy_body_dev(kmx_merge_result* r, uint32_t task, void* dev_dst, uint64_t dst_bytes);
int kmx_result_copy_stats(kmx_merge_result* r, uint32_t task, uint64_t* host_stats /* 6 * n_lists */);
void kmx_result_free(kmx_merge_result* r);

/* kmx_merge_dev with HOST list pointers (what a merge task that has just read its count files holds): the
 * lists are uploaded on a stream of their own -- in ONE copy when they lie back to back in one buffer, best a
 * pinned one (kmx_alloc_pinned) -- so a batch travels while the previous one merges; the host buffers may be
 * reused once kmx_result_wait has returned.  Results are read with the kmx_result_* calls above. */
int kmx_merge_host(kmx_ctx* ctx, const kmx_merge_task* tasks, uint32_t n_tasks, kmx_merge_result** out);
/* page-locked host memory for list buffers / result bodies (plain malloc memory works too, slower) */
void* kmx_alloc_pinned(size_t bytes);
void  kmx_free_pinned(void* p);

/* Host-buffer convenience around kmx_merge_dev for ONE task: lists[i].recs are
 * HOST pointers; uploads, merges, returns the body in a buffer to release with
 * kmx_free.  stats may be NULL. */
int kmx_merge(kmx_ctx* ctx, const kmx_merge_task* task, void** body, uint64_t* body_bytes,
              uint64_t* rows, uint64_t* stats);

/* ----------------------------------------------------------------- filter */

/* `kmtricks filter`: which rows of an existing k-mer matrix does a new sample share (km::FilterTask, matrix.hpp:23-393).
 * rows: n_rows rows of one partition's .count / .pa matrix body in file order -- keys strictly ascending (most significant
 * word first), each row key_words * 8 key bytes (low word first) + 4 * n_cols bytes of u32 counts (KMX_MODE_COUNT) or
 * ceil(n_cols / 8) bytes (KMX_MODE_PA).  key: the new sample's count list of the same partition (a kmx_list: what
 * kmx_count_reads_dev leaves in a kmx_store).  The outputs, by definition:
 *   KMX_FILTER_M  the rows whose k-mer is in `key`, in file order; count rows get one more u32 column at their end, the k-mer's
 *                 count in `key` (row bytes + 4); PA rows are unchanged (f_pa_matrix, matrix.hpp:202-335, writes the bits it read)
 *   KMX_FILTER_V  one u32 per input row: the count in `key` (count rows) or 1 (PA rows) when the row's k-mer is in `key`, else 0
 *   KMX_FILTER_K  the records of `key` whose k-mer is in no row, ascending
 * A run of rows of a partition may be filtered on its own against the whole key list: `marks` (key.n bytes, zeroed by the caller
 * before the first run) carries which records have met a row from call to call; every call adds its own, and a call that asks for
 * KMX_FILTER_K gets the records without a mark as the marks stand after it -- ask in the last run.  M and V of the runs concatenate
 * to M and V of the whole.  marks == NULL: the call holds the whole partition (libkmx keeps the marks itself).
 * LIMITS: a row (with its new column) below 4 GiB; at most 2^32 - 256 rows a call and as many records in the key list; the key
 * list 4-byte aligned; n_cols is otherwise free (no row is ever held in LDS).  Hash matrices and the Bloom modes: KMX_E_UNSUPPORTED. */
#define KMX_FILTER_M 1u
#define KMX_FILTER_V 2u
#define KMX_FILTER_K 4u
typedef struct {
  uint32_t    key_words;      /* ceil(k / 32): 1 ... 4 */
  uint32_t    mode;           /* KMX_MODE_COUNT | KMX_MODE_PA */
  uint32_t    n_cols;         /* N: samples of the matrix */
  uint32_t    want;           /* KMX_FILTER_M | KMX_FILTER_V | KMX_FILTER_K, at least one */
  const void* rows;
  uint64_t    n_rows;
  kmx_list    key;
  uint8_t*    marks;          /* NULL, or key.n bytes: where `key` lies (device memory for kmx_filter_dev) */
  uint32_t    key_on_device;  /* kmx_filter_host only: non-zero = key.recs (and marks) are DEVICE pointers already (a list of a kmx_store) */
} kmx_filter_task;

typedef struct kmx_filter_result kmx_filter_result;

/* key.n zeroed mark bytes in device memory for a partition that is filtered in runs of rows (any n; kmx_filter_marks_free gives them back) */
uint8_t* kmx_filter_marks_alloc(kmx_ctx* ctx, uint64_t n);
void     kmx_filter_marks_free(kmx_ctx* ctx, uint8_t* marks);

/* every pointer of the task a DEVICE pointer; the kernels are queued on the context's stream (kmx_stream) and the call returns;
 * the result (M, V, K as asked for) stays in HBM until it is freed, the call's scratch returns to the context's pool in
 * kmx_filter_result_wait */
int kmx_filter_dev(kmx_ctx* ctx, const kmx_filter_task* task, kmx_filter_result** out);
/* HOST pointers (see key_on_device): the rows (and the key) are uploaded on a stream of their own, so a run travels while the run
 * before it is filtered; host marks are brought back too.  The host buffers may be reused once kmx_filter_result_wait has returned. */
int kmx_filter_host(kmx_ctx* ctx, const kmx_filter_task* task, kmx_filter_result** out);
int      kmx_filter_result_wait(kmx_filter_result* r);
/* (the accessors below wait for the call themselves; what was not asked for is empty: 0 rows / entries / records) */
uint64_t kmx_filter_result_rows(kmx_filter_result* r);             /* kept rows */
uint64_t kmx_filter_result_row_bytes(const kmx_filter_result* r);  /* bytes of a row of M */
uint64_t kmx_filter_result_body_bytes(kmx_filter_result* r);       /* rows * row_bytes when M was asked for */
const void* kmx_filter_result_body_dev(kmx_filter_result* r);
int      kmx_filter_result_copy_body(kmx_filter_result* r, void* host_dst, uint64_t dst_bytes);
uint64_t kmx_filter_result_vector_len(const kmx_filter_result* r); /* n_rows when V was asked for */
const void* kmx_filter_result_vector_dev(kmx_filter_result* r);
int      kmx_filter_result_copy_vector(kmx_filter_result* r, uint32_t* host_dst, uint64_t dst_entries);
uint64_t kmx_filter_result_absent(kmx_filter_result* r);           /* records of K */
const void* kmx_filter_result_absent_dev(kmx_filter_result* r);
int      kmx_filter_result_copy_absent(kmx_filter_result* r, void* host_dst, uint64_t dst_bytes);
/* duration in ms of the call's kernels, for kmx_filter_host with marks their way back included (needs kmx_set_profiling(ctx, 1));
 * < 0 if unavailable */
double   kmx_filter_result_kernel_ms(kmx_filter_result* r);
/* algorithmic bytes: the rows' keys and the key list read, the kept rows in and out (M), the vector (V), the absent records (K) --
 * not the rows that are dropped: the match touches their key only */
uint64_t kmx_filter_result_algo_bytes(kmx_filter_result* r);
void     kmx_filter_result_free(kmx_filter_result* r);

/* ---------------------------------------------------------------- combine */

/* `kmtricks combine`: the matrices of several runs that share a repartition, joined by key (km::MatrixMerger / PartitionMerger,
 * matrix.hpp:396-886).  A task is ONE partition (or one key range of it): n_blocks blocks in column order.  Block i: n_rows rows,
 * keys strictly ascending (most significant word first), each row key_words * 8 key bytes (low word first) and
 *   KMX_MODE_COUNT  n_cols counts of count_bytes (1, 2 or 4) bytes, little endian -- a matrix body has 4-byte counts, the body of a
 *                   .kmer count file is a one-column block of 1-, 2- or 4-byte counts
 *   KMX_MODE_PA     ceil(n_cols / 8) bytes, column j = bit j & 7 of byte j >> 3; the padding bits of the last byte are ignored
 *                   (count_bytes is not read)
 * The output: one row per distinct key of the union of the blocks, ascending; with N = the sum of the blocks' columns and pos_i =
 * the columns of the blocks in front of block i,
 *   KMX_MODE_COUNT  key + N u32: column pos_i + c = block i's count c widened to 32 bits, 0 where block i lacks the key
 *   KMX_MODE_PA     key + ceil(N / 8) bytes: bit pos_i + c = block i's bit c (pos_i need not be a multiple of 8), 0 where block i
 *                   lacks the key; the padding bits of the last byte are 0
 * KMX_COMBINE_DROP_LAST (what PartitionMerger::next does, matrix.hpp:534-583): the greatest key of the union is not written when
 * exactly one block holds it; it is written when two or more do.  Decided on the device.
 * Example (COUNT, one-word keys): block 0, 2 columns, rows 3:(1,2) 9:(5,6); block 1, 1 column of 1-byte counts, rows 3:(7) 4:(8)
 * -> 3:(1,2,7) 4:(0,0,8) 9:(5,6,0); with KMX_COMBINE_DROP_LAST the row of key 9 is missing.
 * Hash matrices are blocks of key_words = 1.  `rows` pointers need no alignment (a 1-byte-count .kmer body has 9-byte rows).
 * Empty blocks and a task of empty blocks are legal (0 rows); a task of one block copies and widens it, clears the PA padding and
 * honours KMX_COMBINE_DROP_LAST.
 * LIMITS, each refused before any GPU work: 1 <= n_blocks <= KMX_COMBINE_MAX_BLOCKS (KMX_E_INVAL / KMX_E_UNSUPPORTED); key_words
 * 1 ... 4, mode COUNT or PA, count_bytes 1, 2 or 4 for COUNT, at least one column a block (KMX_E_INVAL; Bloom modes
 * KMX_E_UNSUPPORTED); at most 2^32 - 256 rows a block and as many in the output -- the output's rows are known on the device
 * only, so the test is on their bound, the blocks' rows together; an input or output row below 4 GiB (KMX_E_UNSUPPORTED).
 * Scratch, from the context's pool until kmx_combine_result_wait gives it back: 8 * key_words + 4 * n_blocks bytes per input row;
 * and the output is sized for the bound of its rows, the blocks' rows together (the call does not wait for the true count).  A
 * call on large bodies already in HBM can therefore return KMX_E_NOMEM although its true output would fit: combine such a
 * partition in key ranges, as `kmx combine --gpus` does. */
#define KMX_COMBINE_DROP_LAST 1u
#define KMX_COMBINE_MAX_BLOCKS 64u
typedef struct {
  const void* rows;
  uint64_t    n_rows;
  uint32_t    n_cols;
  uint32_t    count_bytes;     /* KMX_MODE_COUNT: 1, 2 or 4 */
} kmx_block;
typedef struct {
  uint32_t key_words, mode, n_blocks, flags;
  const kmx_block* blocks;          /* [n_blocks], column order */
  const uint8_t*   block_on_device; /* kmx_combine_host only: NULL, or [n_blocks], non-zero = rows is a DEVICE pointer */
} kmx_combine_task;

typedef struct kmx_combine_result kmx_combine_result;

/* every rows pointer a DEVICE pointer -- kmx_result_body_dev of a COUNT / PA merge result, kmx_filter_result_body_dev, another
 * combine's body, the caller's own memory.  The kernels are queued on the context's stream (kmx_stream), behind whatever produced
 * those bodies there, and the call returns without waiting; the result stays in HBM until it is freed. */
int kmx_combine_dev(kmx_ctx* ctx, const kmx_combine_task* task, kmx_combine_result** out);
/* HOST pointers (see block_on_device): the blocks are uploaded on a stream of their own, so a task travels while the task before
 * it is combined.  The host buffers may be reused once kmx_combine_result_wait has returned. */
int kmx_combine_host(kmx_ctx* ctx, const kmx_combine_task* task, kmx_combine_result** out);
int      kmx_combine_result_wait(kmx_combine_result* r);
/* (the accessors below wait for the call themselves) */
uint64_t kmx_combine_result_rows(kmx_combine_result* r);
uint64_t kmx_combine_result_row_bytes(const kmx_combine_result* r);
uint64_t kmx_combine_result_body_bytes(kmx_combine_result* r);      /* rows * row_bytes */
const void* kmx_combine_result_body_dev(kmx_combine_result* r);
int      kmx_combine_result_copy_body(kmx_combine_result* r, void* host_dst, uint64_t dst_bytes);
/* duration in ms of the call's kernels, the clearing of their tables included (needs kmx_set_profiling(ctx, 1)); < 0 if unavailable */
double   kmx_combine_result_kernel_ms(kmx_combine_result* r);
/* algorithmic bytes: every input row read once plus every output row written once */
uint64_t kmx_combine_result_algo_bytes(kmx_combine_result* r);
void     kmx_combine_result_free(kmx_combine_result* r);

/* ------------------------------------------------------------------ query */

/* Which samples of a Bloom matrix hold the k-mers of a query sequence (what kmtricks 1.0 shipped as `kmtricks query` and kmindex
 * does today; the addressing is the published one: repartition.hpp:94-103 get_partition, kmer_hash.hpp:244-328 WinHasher).
 * The index: the .cmbf bodies of a `--mode hash:bf:bin` run -- per partition `window` rows of ceil(n_cols / 8) bytes, sample i = bit
 * i & 7 of byte i >> 3.  For every query q (read q = bases[offsets[q] .. offsets[q + 1]), as in kmx_count_reads) and every position
 * whose k bases are all ACGT (either case): c = the canonical k-mer (A0 C1 T2 G3, min(forward, reverse complement)), p =
 * repart[minimizer(c)] (the split's minimizer), h = XXH64(c's ceil(k / 32) words, seed 0) % window (kmx_count_hash without the
 * partition offset), row = rows[p] + h * ceil(n_cols / 8).  Results: n_kmers[q] = such positions; hits[q * n_cols + i] = those whose
 * row has bit i set.  Every occurrence counts; a row's padding bits are never read into a result; a query without a valid k-mer has
 * zeros and is still reported.
 * rows: a HOST array of nb_parts pointers to matrix bodies; NULL = the partition is not part of this call (its k-mers count in
 * n_kmers and add no hits).  hits: NULL (the result owns a zeroed table), or a DEVICE table of n_seqs * n_cols u32 that the call ADDS
 * to: the partition groups of one set of queries accumulate on the device (u32 adds commute: the table does not depend on order).
 * LIMITS, each refused before any GPU work: 8 <= kmer_size <= 127, 4 <= minim_size <= 15 and < kmer_size, 1 <= nb_parts <= 65535
 * (KMX_E_INVAL); window 1 ... 2^32 - 1, fewer than 2^31 queries and fewer than 2^32 bases a call -- so no query has 2^32 positions
 * or more, the counters are u32 -- (KMX_E_UNSUPPORTED: send the queries in batches).
 * Scratch from the context's pool: 16 bytes a base. */
typedef struct {
  const char*     bases;
  const uint64_t* offsets;      /* [n_seqs + 1], offsets[0] = 0 */
  uint64_t        n_seqs;
  uint32_t        kmer_size, minim_size;
  const uint16_t* repart;       /* u16[4^minim_size]: minimizer -> partition */
  uint32_t        nb_parts;
  uint32_t        n_cols;       /* N: samples (bits of a row) */
  uint64_t        window;       /* W: rows of a partition's matrix */
  const uint8_t* const* rows;   /* [nb_parts] */
  uint32_t*       hits;         /* NULL, or a device table to accumulate into */
} kmx_query_task;

typedef struct kmx_query_result kmx_query_result;

/* bases, offsets, repart and every rows[p] DEVICE pointers (the rows array itself lies in host memory).  The kernels are queued on the
 * context's stream (kmx_stream) and the call returns; it reads offsets[n_seqs] back first (8 bytes: the grid's size).  The result
 * stays in HBM until it is freed. */
int kmx_query_dev(kmx_ctx* ctx, const kmx_query_task* task, kmx_query_result** out);
/* HOST pointers (hits, when given, is still a device table): everything is uploaded on a stream of its own, so a call's inputs travel
 * while the call before it runs.  The host buffers may be reused once kmx_query_result_wait has returned. */
int kmx_query_host(kmx_ctx* ctx, const kmx_query_task* task, kmx_query_result** out);
int      kmx_query_result_wait(kmx_query_result* r);
/* (the accessors below wait for the call themselves) */
uint64_t kmx_query_result_n_seqs(const kmx_query_result* r);
int      kmx_query_result_copy_kmers(kmx_query_result* r, uint32_t* host_dst, uint64_t dst_entries);   /* n_seqs entries */
int      kmx_query_result_copy_hits(kmx_query_result* r, uint32_t* host_dst, uint64_t dst_entries);    /* n_seqs * n_cols: the table as it stands, the task's when one was given */
uint32_t* kmx_query_result_hits_dev(kmx_query_result* r);
/* duration in ms of the call's kernels, the clearing of their tables included (needs kmx_set_profiling(ctx, 1)); < 0 if unavailable */
double   kmx_query_result_kernel_ms(kmx_query_result* r);
/* algorithmic bytes: the bases read + one row per valid k-mer of a partition that is part of the call or not (n_kmers * ceil(n_cols / 8))
 * + the hits table written */
uint64_t kmx_query_result_algo_bytes(kmx_query_result* r);
void     kmx_query_result_free(kmx_query_result* r);

/* ----------------------------------------------------------------- kquery */

/* Which samples of a K-MER matrix hold the k-mers of a query sequence, and how often: exact, where kmx_query_* answers from Bloom
 * matrices.  The index: the .count / .pa bodies of a `--mode kmer:count:bin` / `kmer:pa:bin` run -- partition p has n_rows[p] rows in
 * file order, keys strictly ascending (most significant word first), a row laid out as in the filter section above: key_words * 8 key
 * bytes (low word first), then 4 * n_cols bytes of u32 counts (KMX_MODE_COUNT) or ceil(n_cols / 8) bytes, column i = bit i & 7 of byte
 * i >> 3 (KMX_MODE_PA).  For every query q and every position whose k bases are all ACGT (either case) and whose k-mer ends inside
 * the query: c = the canonical k-mer, p = repart[minimizer(c)], both exactly as the query section defines them.  Results:
 *   n_kmers[q]           the number of such positions
 *   hits[q * n_cols + i] (u32) the number of them for which c is the key of a row of partition p and that row's count i is non-zero
 *                        (COUNT) or its bit i is set (PA)
 *   sums[q * n_cols + i] (u64; COUNT, with want_sums) the sum of that row's count i over the same positions
 * Every occurrence counts; the padding bits of a PA row never reach a result; a query without a valid k-mer has zeros and is still
 * reported.  rows: a HOST array of nb_parts pointers; NULL = the partition is not part of this call (its k-mers count in n_kmers and
 * add nothing else; n_rows[p] is not read).  n_rows: a HOST array in both calls.  hits / sums: NULL (the result owns a zeroed table;
 * sums only with want_sums), or DEVICE tables of n_seqs * n_cols entries that the call ADDS to: the partition groups of one set of
 * queries accumulate on the device (integer adds commute: the tables do not depend on order).
 * LIMITS, each refused before any GPU work: 8 <= kmer_size <= 127, 4 <= minim_size <= 15 and < kmer_size, key_words == ceil(kmer_size
 * / 32), 1 <= nb_parts <= 65535, n_cols >= 1, mode COUNT or PA, want_sums (or a sums table) with PA, a sums table without want_sums
 * (KMX_E_INVAL); fewer than 2^31 queries and fewer than 2^32 bases a call, at most 2^32 - 256 rows a partition, a row below 4 GiB,
 * the Bloom modes -- and hash matrices, which no field tells apart: they are not k-mer matrices -- (KMX_E_UNSUPPORTED).
 * Scratch from the context's pool: 10 + 8 * key_words bytes a base (the partition, the canonical words, one record). */
typedef struct {
  const char*     bases;
  const uint64_t* offsets;      /* [n_seqs + 1], offsets[0] = 0 */
  uint64_t        n_seqs;
  uint32_t        kmer_size, minim_size;
  const uint16_t* repart;       /* u16[4^minim_size]: minimizer -> partition */
  uint32_t        nb_parts;
  uint32_t        n_cols;       /* N: samples of the matrix */
  uint32_t        key_words;    /* ceil(kmer_size / 32) */
  uint32_t        mode;         /* KMX_MODE_COUNT | KMX_MODE_PA */
  const uint64_t* n_rows;       /* HOST [nb_parts]: rows of every partition's matrix */
  const uint8_t* const* rows;   /* HOST [nb_parts] */
  uint32_t*       hits;         /* NULL, or a device table to accumulate into */
  uint64_t*       sums;         /* NULL, or (with want_sums) a device table to accumulate into */
  uint32_t        want_sums;    /* non-zero: the sums are computed (KMX_MODE_COUNT only) */
} kmx_kquery_task;

typedef struct kmx_kquery_result kmx_kquery_result;

/* bases, offsets, repart and every rows[p] DEVICE pointers.  The kernels are queued on the context's stream (kmx_stream) and the call
 * returns; it reads offsets[n_seqs] back first (8 bytes: the grid's size).  The results stay in HBM until they are freed. */
int kmx_kquery_dev(kmx_ctx* ctx, const kmx_kquery_task* task, kmx_kquery_result** out);
/* HOST pointers (hits and sums, when given, are still device tables): everything is uploaded on a stream of its own.  The host
 * buffers may be reused once kmx_kquery_result_wait has returned. */
int kmx_kquery_host(kmx_ctx* ctx, const kmx_kquery_task* task, kmx_kquery_result** out);
int      kmx_kquery_result_wait(kmx_kquery_result* r);
/* (the accessors below wait for the call themselves) */
uint64_t kmx_kquery_result_n_seqs(const kmx_kquery_result* r);
int      kmx_kquery_result_copy_kmers(kmx_kquery_result* r, uint32_t* host_dst, uint64_t dst_entries);   /* n_seqs entries */
int      kmx_kquery_result_copy_hits(kmx_kquery_result* r, uint32_t* host_dst, uint64_t dst_entries);    /* n_seqs * n_cols: the table as it stands */
int      kmx_kquery_result_copy_sums(kmx_kquery_result* r, uint64_t* host_dst, uint64_t dst_entries);    /* n_seqs * n_cols; KMX_E_INVAL without want_sums */
uint32_t* kmx_kquery_result_hits_dev(kmx_kquery_result* r);
uint64_t* kmx_kquery_result_sums_dev(kmx_kquery_result* r);     /* NULL without want_sums */
/* duration in ms of the call's kernels, the clearing of their tables included (needs kmx_set_profiling(ctx, 1)); < 0 if unavailable */
double   kmx_kquery_result_kernel_ms(kmx_kquery_result* r);
/* algorithmic bytes: the bases read + one row (key and payload) per k-mer that met a row + the probes' keys (8 * key_words per valid
 * k-mer) + the tables written */
uint64_t kmx_kquery_result_algo_bytes(kmx_kquery_result* r);
void     kmx_kquery_result_free(kmx_kquery_result* r);

/* ----------------------------------------------------------------- zquery */

/* The findere trick over the Bloom matrices of the query section: the index stays as it is, with k-mers of the run's k; the query asks
 * for (k + z)-mers.  A (k + z)-mer is present in a sample only when all of its z + 1 overlapping k-mers are: a false positive needs
 * z + 1 Bloom errors in a row.  Everything of the query section stands: the index, what a valid position is, the canonical k-mer, the
 * partition, the row, the masking of padding bits.  Let K = kmer_size + z.  Position j of query q is a K-POSITION when j + K <= the
 * query's end and all K bases from j on are ACGT (either case) -- positions j and j + z are both valid k-mer positions of q.  Results:
 *   n_kmers[q]           the number of K-positions of q
 *   hits[q * n_cols + i] the number of K-positions j for which bit i is set in the row of EVERY k-mer at j, j + 1, ..., j + z
 * Every occurrence counts; z = 0 is the query section's result, bit for bit.
 * A SERIES is one or more calls over the same bases and offsets, each with a different set of non-NULL rows[p] (the partition groups
 * of an index that does not fit the device), all sharing one `bits` table: per base one row of kmx_zquery_bits_bytes(1, n_cols) bytes,
 * the k-mer's matrix row at that position masked to the columns below n_cols (zeros where no k-mer is or its partition was in no call).
 * The first call passes bits = NULL and its result owns a zeroed table (kmx_zquery_result_bits_dev; the result is kept until the
 * series has ended); the later calls pass that table.  The call with last != 0 ends the series: it runs the window pass over the table
 * and produces n_kmers and hits.  A k-mer whose partition is in no call of the series has a row of zeros: its windows count in n_kmers
 * and add no hit.  A single call with every partition and last = 1 is the common case.  hits: NULL (the last call's result owns a
 * zeroed table) or a DEVICE table of n_seqs * n_cols u32 that the window pass ADDS to; read only when last.
 * LIMITS, each refused before any GPU work: the query section's; z > 8 or z >= kmer_size (KMX_E_INVAL); a bits table of more than
 * 2^40 bytes (KMX_E_UNSUPPORTED: send the queries in batches).
 * Scratch from the context's pool: 16 bytes a base, plus the bits table when the result owns it. */
typedef struct {
  const char*     bases;
  const uint64_t* offsets;      /* [n_seqs + 1], offsets[0] = 0 */
  uint64_t        n_seqs;
  uint32_t        kmer_size, minim_size;
  const uint16_t* repart;       /* u16[4^minim_size]: minimizer -> partition */
  uint32_t        nb_parts;
  uint32_t        n_cols;       /* N: samples (bits of a row) */
  uint64_t        window;       /* W: rows of a partition's matrix */
  const uint8_t* const* rows;   /* [nb_parts] */
  uint32_t        z;            /* 0 ... 8 and below kmer_size */
  uint32_t        last;         /* non-zero: this call ends the series: the window pass runs, n_kmers and hits are produced */
  uint8_t*        bits;         /* NULL: the result owns a zeroed table; else a DEVICE table from an earlier call of the series */
  uint32_t*       hits;         /* NULL, or a device table the window pass adds to; read only when last */
} kmx_zquery_task;

typedef struct kmx_zquery_result kmx_zquery_result;

/* bytes of the bits table of n_bases bases: n_bases * pitch, pitch = 4 * ceil(ceil(n_cols / 8) / 4) */
uint64_t kmx_zquery_bits_bytes(uint64_t n_bases, uint32_t n_cols);
/* bases, offsets, repart, every rows[p], bits and hits DEVICE pointers (the rows array itself lies in host memory).  The kernels are
 * queued on the context's stream and the call returns; it reads offsets[n_seqs] back first (8 bytes: the grid's size). */
int kmx_zquery_dev(kmx_ctx* ctx, const kmx_zquery_task* task, kmx_zquery_result** out);
/* HOST pointers (bits and hits, when given, are still device tables): everything is uploaded on a stream of its own.  The host buffers
 * may be reused once kmx_zquery_result_wait has returned. */
int kmx_zquery_host(kmx_ctx* ctx, const kmx_zquery_task* task, kmx_zquery_result** out);
int      kmx_zquery_result_wait(kmx_zquery_result* r);
/* (the accessors below wait for the call themselves) */
uint64_t kmx_zquery_result_n_seqs(const kmx_zquery_result* r);
/* n_kmers and hits exist once the series has ended: on the result of a call without `last` the copies return KMX_E_INVAL, hits_dev NULL */
int      kmx_zquery_result_copy_kmers(kmx_zquery_result* r, uint32_t* host_dst, uint64_t dst_entries);   /* n_seqs entries */
int      kmx_zquery_result_copy_hits(kmx_zquery_result* r, uint32_t* host_dst, uint64_t dst_entries);    /* n_seqs * n_cols: the table as it stands, the task's when one was given */
uint32_t* kmx_zquery_result_hits_dev(kmx_zquery_result* r);
uint8_t* kmx_zquery_result_bits_dev(kmx_zquery_result* r);      /* the series' table: the result's own or the task's */
/* duration in ms of the call's kernels, the clearing of their tables included (needs kmx_set_profiling(ctx, 1)); < 0 if unavailable */
double   kmx_zquery_result_kernel_ms(kmx_zquery_result* r);
/* algorithmic bytes, with found = the call's valid k-mers whose partition is part of the call, nb = ceil(n_cols / 8) and pitch as above:
 * the bases read + found * nb (rows read) + found * pitch (table rows written); and for the last call + (K-positions + z per query
 * that has any) * pitch (table rows read by the window pass) + 4 * n_seqs * n_cols (the hits table written) */
uint64_t kmx_zquery_result_algo_bytes(kmx_zquery_result* r);
void     kmx_zquery_result_free(kmx_zquery_result* r);

/* ----------------------------------------------------------------- cquery */

/* Which samples of a COUNTING Bloom matrix hold the k-mers of a query sequence, and at what abundance (what kmindex asks of kmtricks'
 * --bitw indexes; no counterpart in the 1.6.0 tree).
 * THE INDEX: the .cmbf bodies of a `--mode hash:bfc:bin` run -- per partition `window` rows of nb = ceil(N * w / 8) bytes, N = n_cols,
 * w = bitw (the header's `bits` field is N * w).  Bit position t of a row is bit 7 - (t & 7) of byte t >> 3 (bitpacker's MSB-first
 * order, as the merge writes it).  Sample i's CLASS v_i is the w bits at positions i * w ... i * w + w - 1, the first of them the most
 * significant: v_i = (R >> (8 * nb - (i + 1) * w)) & (2^w - 1) with R the row read as one big-endian number.  The merge writes
 * v = min(bit_length(count), 2^w - 1).  The padding bits behind position N * w never reach a result.
 * ADDRESSING: exactly the query section's -- what a valid position is, the canonical k-mer c, p = repart[minimizer(c)], h = XXH64(c) %
 * window, row = rows[p] + h * nb, NULL partitions, every occurrence counts.
 * floor_of(v) = 0 for v = 0, else 2^(min(v, 32) - 1): the smallest count the merge maps to class v.  For the top class 2^w - 1 it is a
 * LOWER BOUND only (every count of that bit length and above lands there).  The clamp at 32: a count is a u32, so a class above 32
 * stands only in a body no merge wrote, and such a body is still answered without overflow.
 * RESULTS per query q and column i:
 *   n_kmers[q]           the valid positions, as in the query section
 *   hits[q * n_cols + i] (u32) the positions whose v_i >= min_class
 *   sums[q * n_cols + i] (u64) the sum of floor_of(v_i) over all valid positions of q whose partition is part of the call; it does not
 *                        depend on min_class
 * hits and sums: both NULL (the result owns zeroed tables) or both DEVICE tables of n_seqs * n_cols entries that the call ADDS to (one
 * without the other: KMX_E_INVAL); the partition groups of one set of queries accumulate on the device in any order.
 * EXAMPLES.  w = 3, N = 3: nb = 2, the third field lies across the two bytes, 7 padding bits (here all set) follow it.
 *   row 22 FF: bits 001 000 101 -> classes (1, 0, 5), floors (1, 0, 16)
 *   row ED 7F: bits 111 011 010 -> classes (7, 3, 2), floors (64, 4, 2)      (7 is the top class: counts of 64 and above)
 *   row 1B FF: bits 000 110 111 -> classes (0, 6, 7), floors (0, 32, 64)
 * A query whose three valid positions meet these three rows: min_class 1 gives hits (2, 2, 3), min_class 4 gives hits (1, 1, 2), both
 * give sums (65, 36, 82).  At w = 8 a byte FF is class 255, clamped: floor 2^31.
 * LIMITS, each refused before any GPU work: the query section's, unchanged; bitw 0 or above 32, min_class outside 1 ... 2^bitw - 1
 * (KMX_E_INVAL); bitw 9 ... 32 -- a class never exceeds 32, so 6 bits hold every class and 8 keep a field inside two bytes --, a row of
 * 4 GiB or more, n_seqs * n_cols >= 2^61 (KMX_E_UNSUPPORTED).
 * Scratch from the context's pool: 16 bytes a base. */
typedef struct {
  const char*     bases;
  const uint64_t* offsets;      /* [n_seqs + 1], offsets[0] = 0 */
  uint64_t        n_seqs;
  uint32_t        kmer_size, minim_size;
  const uint16_t* repart;       /* u16[4^minim_size]: minimizer -> partition */
  uint32_t        nb_parts;
  uint32_t        n_cols;       /* N: samples (fields of a row) */
  uint64_t        window;       /* W: rows of a partition's matrix */
  const uint8_t* const* rows;   /* [nb_parts] */
  uint32_t        bitw;         /* w: bits of a field, 1 ... 8 */
  uint32_t        min_class;    /* a hit is a class of at least this: 1 ... 2^bitw - 1 */
  uint32_t*       hits;         /* NULL, or a device table to accumulate into */
  uint64_t*       sums;         /* NULL with hits, or a device table to accumulate into */
} kmx_cquery_task;

typedef struct kmx_cquery_result kmx_cquery_result;

/* bases, offsets, repart and every rows[p] DEVICE pointers (the rows array itself lies in host memory).  The kernels are queued on the
 * context's stream (kmx_stream) and the call returns; it reads offsets[n_seqs] back first (8 bytes: the grid's size).  The results
 * stay in HBM until they are freed; the call's scratch returns to the pool in kmx_cquery_result_wait. */
int kmx_cquery_dev(kmx_ctx* ctx, const kmx_cquery_task* task, kmx_cquery_result** out);
/* HOST pointers (hits and sums, when given, are still device tables): everything is uploaded on a stream of its own.  The host buffers
 * may be reused once kmx_cquery_result_wait has returned. */
int kmx_cquery_host(kmx_ctx* ctx, const kmx_cquery_task* task, kmx_cquery_result** out);
int      kmx_cquery_result_wait(kmx_cquery_result* r);
/* (the accessors below wait for the call themselves) */
uint64_t kmx_cquery_result_n_seqs(const kmx_cquery_result* r);
int      kmx_cquery_result_copy_kmers(kmx_cquery_result* r, uint32_t* host_dst, uint64_t dst_entries);   /* n_seqs entries */
int      kmx_cquery_result_copy_hits(kmx_cquery_result* r, uint32_t* host_dst, uint64_t dst_entries);    /* n_seqs * n_cols: the table as it stands */
int      kmx_cquery_result_copy_sums(kmx_cquery_result* r, uint64_t* host_dst, uint64_t dst_entries);    /* n_seqs * n_cols: the table as it stands */
uint32_t* kmx_cquery_result_hits_dev(kmx_cquery_result* r);
uint64_t* kmx_cquery_result_sums_dev(kmx_cquery_result* r);
/* duration in ms of the call's kernels, the clearing of their tables included (needs kmx_set_profiling(ctx, 1)); < 0 if unavailable */
double   kmx_cquery_result_kernel_ms(kmx_cquery_result* r);
/* algorithmic bytes: the bases read + one row per valid k-mer of a partition that is part of the call or not (n_kmers * nb) + both
 * tables written (12 * n_seqs * n_cols) */
uint64_t kmx_cquery_result_algo_bytes(kmx_cquery_result* r);
void     kmx_cquery_result_free(kmx_cquery_result* r);

/* ------------------------------------------------------------------- dist */

/* How the samples of a matrix relate to each other: the shared k-mer tables that the Jaccard and Bray-Curtis distances follow from
 * (what Simka computes on the CPU).  Input: a run of n_rows rows of ONE partition's matrix body, n_cols = N samples:
 *   key_words 1 ... 4, KMX_MODE_PA     a row is 8 * key_words key bytes, then ceil(N / 8) bytes, column i = bit i & 7 of byte i >> 3
 *                                      (.pa and .pa_hash bodies)
 *   key_words 1 ... 4, KMX_MODE_COUNT  a row is the key, then N u32 counts; column i is present when its count is non-zero
 *                                      (.count and .count_hash bodies)
 *   key_words 0,       KMX_MODE_BF     a row is ceil(N / 8) bytes and has no key (.cmbf bodies)
 * Keys are never read.  The padding bits of a row's last byte never reach a result.  `rows` needs no alignment (a PA row of a
 * one-word key and 13 bytes is 21 bytes long).  Outputs: N x N tables of u64, row-major, the full square with both triangles written:
 *   inter[i * N + j]  the number of rows in which columns i and j are both present; the diagonal is the number of rows that hold sample i
 *   mins[i * N + j]   (COUNT with want_mins only) the sum over the rows of min(count_i, count_j); the diagonal is the sum of sample i's counts
 * The call ADDS to the tables it is given: inter / mins are NULL (the result owns a zeroed table) or DEVICE tables of N * N u64.  The
 * partitions of a run, and the row runs of a partition, accumulate on the device in any order: integer adds commute, so the tables depend
 * neither on the order nor on how the rows were cut.  n_rows = 0 is legal and adds nothing.
 * Examples.  PA, N = 3, rows with bits (column 0 = bit 0) 0b011, 0b101, 0b111, 0b000: inter = [[3,2,2],[2,2,1],[2,1,2]].
 * COUNT, rows (1,2,0), (5,0,7), (3,3,3): the same inter; mins = [[9,4,8],[4,5,3],[8,3,10]]; the Jaccard distance of samples 0 and 1 is
 * 1 - 2 / (3 + 2 - 2) = 0.333333, their Bray-Curtis distance 1 - 2 * 4 / (9 + 5) = 0.428571.
 * LIMITS, each refused before any GPU work.  KMX_E_INVAL: n_cols = 0; a mode other than COUNT, PA or BF; key_words > 4; key_words = 0
 * with a mode other than BF; BF with key_words != 0; want_mins, or a mins table, outside COUNT; a mins table without want_mins.
 * KMX_E_UNSUPPORTED: n_cols > 32768 (a table would be 8 GiB); a row of 4 GiB or more; KMX_MODE_BFC and KMX_MODE_BFT.
 * Scratch from the context's pool: round_up64(N) / 8 bytes per row (rows rounded up to 64) -- the presence bits, sample-major in blocks
 * of 64 samples, which the pair kernel reads -- and, for kmx_dist_host, the uploaded rows.  Send a body that does not fit in runs of rows. */
typedef struct {
  uint32_t    key_words;     /* 0 (BF) ... 4 */
  uint32_t    mode;          /* KMX_MODE_COUNT | KMX_MODE_PA | KMX_MODE_BF */
  uint32_t    n_cols;        /* N: samples of the matrix */
  uint32_t    want_mins;     /* non-zero: mins is computed (KMX_MODE_COUNT only) */
  const void* rows;
  uint64_t    n_rows;
  uint64_t*   inter;         /* NULL, or a device table to accumulate into */
  uint64_t*   mins;          /* NULL, or (with want_mins) a device table to accumulate into */
} kmx_dist_task;

typedef struct kmx_dist_result kmx_dist_result;

/* every pointer a DEVICE pointer -- rows may be kmx_result_body_dev of a merge result, a filter's or a combine's body, the caller's own
 * memory.  The kernels are queued on the context's stream (kmx_stream), behind whatever produced the rows there, and the call returns
 * without waiting; the tables stay in HBM until the result is freed (tables of the caller's are the caller's). */
int kmx_dist_dev(kmx_ctx* ctx, const kmx_dist_task* task, kmx_dist_result** out);
/* rows a HOST pointer (inter and mins, when given, are still device tables): the rows are uploaded on a stream of their own, so a run
 * travels while the run before it is worked on.  The host buffer may be reused once kmx_dist_result_wait has returned. */
int kmx_dist_host(kmx_ctx* ctx, const kmx_dist_task* task, kmx_dist_result** out);
int       kmx_dist_result_wait(kmx_dist_result* r);
/* (the accessors below wait for the call themselves) */
uint64_t* kmx_dist_result_inter_dev(kmx_dist_result* r);      /* the table as it stands: the result's own or the task's */
uint64_t* kmx_dist_result_mins_dev(kmx_dist_result* r);       /* NULL without want_mins */
int       kmx_dist_result_copy_inter(kmx_dist_result* r, uint64_t* host_dst, uint64_t dst_entries);   /* N * N entries */
int       kmx_dist_result_copy_mins(kmx_dist_result* r, uint64_t* host_dst, uint64_t dst_entries);    /* N * N; KMX_E_INVAL without want_mins */
/* duration in ms of the call's kernels, the clearing of the tables the result owns included (needs kmx_set_profiling(ctx, 1)); < 0 if unavailable */
double    kmx_dist_result_kernel_ms(kmx_dist_result* r);
/* the same interval in its parts: clearing + k_dist_slab, k_dist_pairs, k_dist_mins (-1 without want_mins); any pointer may be NULL */
int       kmx_dist_result_kernel_parts_ms(kmx_dist_result* r, double* slab_ms, double* pairs_ms, double* mins_ms);
/* algorithmic bytes: the body read once (n_rows * row bytes) + the presence bits written and read once (2 * round_up64(N) / 8 *
 * round_up64(n_rows)) + the inter table written (8 * N * N); with want_mins the counts read once more (4 * N * n_rows) and the mins
 * table written */
uint64_t  kmx_dist_result_algo_bytes(kmx_dist_result* r);
void      kmx_dist_result_free(kmx_dist_result* r);

/* ------------------------------------------------------------------- diff */

/* Differential k-mer analysis (what kmdiff does on top of kmtricks; no counterpart in the kmtricks tree): with the samples split into
 * controls and cases, which rows of a matrix are significantly over- or under-represented in one group.
 * INPUT: a run of n_rows rows of ONE partition's matrix body, n_cols = N samples:
 *   key_words 1 ... 4, KMX_MODE_COUNT  a row is 8 * key_words key bytes, then N u32 counts (.count and .count_hash bodies)
 *   key_words 1 ... 4, KMX_MODE_PA     a row is the key, then ceil(N / 8) bytes, column i = bit i & 7 of byte i >> 3 (.pa, .pa_hash);
 *                                      a sample's "count" is its bit
 * `rows` needs no alignment.  The padding bits of a PA row never reach a result.  Keys are never read, only moved.
 * group[N], a HOST array of u8, gives each column its group: 0 control, 1 case, 2 ignored.
 *
 * COLUMN SUMS (kmx_colsums_*): the call ADDS per column the sum of its counts (COUNT) or the number of rows that hold it (PA) into a
 * table of N u64: a DEVICE table of the caller's, or NULL (the result owns a zeroed one).  Partitions and runs of rows accumulate in
 * any order; n_rows = 0 adds nothing.  These are the per-sample totals T_i the test needs.
 *
 * THE TEST (kmx_diff_*): parameters total_ctrl = T0 and total_case = T1 (u64: the sums of T_i over each group, over the whole run),
 * threshold (double), min_rec (u32).  Per row:
 *   c0, c1 (u64)  the sums of the row's counts over the control / case columns
 *   r0, r1 (u32)  the number of control / case columns that are non-zero
 *   over          1 if c1 * T0 > c0 * T1, 2 if c1 * T0 < c0 * T1, 0 if equal -- compared in exact 128-bit integer arithmetic
 *   stat          the Poisson likelihood-ratio statistic of "one rate" against "a rate per group" (the per-sample terms cancel: a
 *                 function of c0, c1, T0, T1 alone).  With c = c0 + c1 and T = T0 + T1:
 *                   stat = max(0, 2 * [ c1 * ln((c1 * T) / (c * T1)) + c0 * ln((c0 * T) / (c * T0)) ])
 *                 a term whose c_g is 0 is 0; c = 0 gives 0.  All products, quotients and logs in IEEE double, evaluated in the order
 *                 written (no fused multiply-add).
 * A row is KEPT iff r0 + r1 >= min_rec and stat >= threshold.  Threshold 0 keeps every row that passes min_rec; +inf keeps none.
 * OUTPUTS: the kept rows whole, in the input's order (a valid body of the same row size); one kmx_diff_rec per kept row in the same
 * order; the count of kept rows.
 * EXAMPLES.  N = 4, groups (0,0,1,1), T0 = T1 = 100:
 *   row (0,0,5,5): c0 = 0, c1 = 10, stat = 20 ln 2 = 13.862943611198906, over = 1
 *   row (3,3,3,3): stat = 0, over = 0
 *   row (1,2,4,8): c0 = 3, c1 = 12, stat ~ 5.7823427, over = 1
 * With threshold 3.841458820694126 (p = 0.05, one degree of freedom) rows 0 and 2 are kept, in that order.  Swapping the groups gives
 * the same stats with over = 2.
 * LIMITS, each refused before any GPU work.  KMX_E_INVAL: n_cols = 0; a mode other than COUNT or PA; key_words 0 or > 4; a group value
 * > 2; no control column or no case column; total_ctrl or total_case = 0 (or their sum at 2^64 and above); a NaN or negative threshold.
 * KMX_E_UNSUPPORTED: KMX_MODE_BF, KMX_MODE_BFC, KMX_MODE_BFT; n_rows > 2^32 - 256 (the placement tiles are the filter's: 256 rows); a
 * row of 4 GiB or more.
 * SCRATCH from the context's pool, per kmx_diff call: a 4-byte keep word and a 40-byte record slot per input row, a 4-byte counter per
 * 256 rows, the group table (N bytes; PA: 2 * ceil(N / 8) bytes of masks) -- all given back when the call has run; the outputs are
 * sized for every row kept (n_rows * row bytes + 16, and 40 * n_rows) and live until the result is freed; for the _host calls the
 * uploaded rows.  kmx_colsums: the table when the result owns it, and the upload.  Send a body that does not fit in runs of rows. */
typedef struct {
  uint32_t    key_words;     /* 1 ... 4 */
  uint32_t    mode;          /* KMX_MODE_COUNT | KMX_MODE_PA */
  uint32_t    n_cols;        /* N: samples of the matrix */
  uint32_t    reserved;      /* 0 */
  const void* rows;
  uint64_t    n_rows;
  uint64_t*   sums;          /* NULL, or a device table of N u64 to accumulate into */
} kmx_colsums_task;

typedef struct {
  uint32_t       key_words;     /* 1 ... 4 */
  uint32_t       mode;          /* KMX_MODE_COUNT | KMX_MODE_PA */
  uint32_t       n_cols;        /* N: samples of the matrix */
  uint32_t       min_rec;       /* a kept row has at least this many non-zero control + case columns */
  const void*    rows;
  uint64_t       n_rows;
  const uint8_t* group;         /* HOST: N bytes, 0 control, 1 case, 2 ignored (copied by the call) */
  uint64_t       total_ctrl;    /* T0 */
  uint64_t       total_case;    /* T1 */
  double         threshold;     /* a kept row has stat >= threshold */
} kmx_diff_task;

typedef struct {
  uint64_t sum_ctrl;     /* c0 */
  uint64_t sum_case;     /* c1 */
  double   stat;
  uint32_t rec_ctrl;     /* r0 */
  uint32_t rec_case;     /* r1 */
  uint32_t row;          /* index in the input */
  uint32_t over;         /* 1 case, 2 control, 0 neither */
} kmx_diff_rec;          /* 40 bytes */

typedef struct kmx_colsums_result kmx_colsums_result;
typedef struct kmx_diff_result kmx_diff_result;

/* _dev: every pointer except `group` a DEVICE pointer -- rows may be kmx_result_body_dev of a merge result, a filter's or a combine's
 * body, the caller's own memory.  The kernels are queued on the context's stream (kmx_stream) and the call returns without waiting.
 * _host: rows a HOST pointer (sums, when given, is still a device table): the rows are uploaded on a stream of their own, so a run
 * travels while the run before it is worked on.  The host buffer may be reused once _result_wait has returned. */
int kmx_colsums_dev(kmx_ctx* ctx, const kmx_colsums_task* task, kmx_colsums_result** out);
int kmx_colsums_host(kmx_ctx* ctx, const kmx_colsums_task* task, kmx_colsums_result** out);
int       kmx_colsums_result_wait(kmx_colsums_result* r);
/* (the accessors below wait for the call themselves) */
uint64_t* kmx_colsums_result_sums_dev(kmx_colsums_result* r);      /* the table as it stands: the result's own or the task's */
int       kmx_colsums_result_copy_sums(kmx_colsums_result* r, uint64_t* host_dst, uint64_t dst_entries);   /* N entries */
double    kmx_colsums_result_kernel_ms(kmx_colsums_result* r);     /* needs kmx_set_profiling(ctx, 1); < 0 if unavailable */
/* algorithmic bytes: the body read once (n_rows * row bytes) + the table (8 * N) */
uint64_t  kmx_colsums_result_algo_bytes(kmx_colsums_result* r);
void      kmx_colsums_result_free(kmx_colsums_result* r);

int kmx_diff_dev(kmx_ctx* ctx, const kmx_diff_task* task, kmx_diff_result** out);
int kmx_diff_host(kmx_ctx* ctx, const kmx_diff_task* task, kmx_diff_result** out);
int       kmx_diff_result_wait(kmx_diff_result* r);
uint64_t  kmx_diff_result_rows(kmx_diff_result* r);                /* kept rows */
uint64_t  kmx_diff_result_row_bytes(const kmx_diff_result* r);
uint64_t  kmx_diff_result_body_bytes(kmx_diff_result* r);          /* rows * row_bytes */
const void*         kmx_diff_result_body_dev(kmx_diff_result* r);  /* the kept rows, in HBM until the result is freed */
int       kmx_diff_result_copy_body(kmx_diff_result* r, void* host_dst, uint64_t dst_bytes);
const kmx_diff_rec* kmx_diff_result_recs_dev(kmx_diff_result* r);
int       kmx_diff_result_copy_recs(kmx_diff_result* r, kmx_diff_rec* host_dst, uint64_t dst_entries);
double    kmx_diff_result_kernel_ms(kmx_diff_result* r);
/* algorithmic bytes: the body read once + the kept rows written + 40 bytes per kept row */
uint64_t  kmx_diff_result_algo_bytes(kmx_diff_result* r);
void      kmx_diff_result_free(kmx_diff_result* r);

/* ----------------------------------------------------------------- select */

/* A smaller matrix out of a larger one (what MUSET's `kmat_tools filter` does on the text of a kmtricks matrix; no counterpart in the
 * kmtricks tree): some of the columns, in any order, and the rows whose recurrence over those columns lies in a range -- as counts or as
 * presence/absence bits.
 * INPUT: a run of n_rows rows of ONE partition's matrix body, n_cols = N samples:
 *   key_words 1 ... 4, KMX_MODE_COUNT  a row is 8 * key_words key bytes, then N u32 counts
 *   key_words 1 ... 4, KMX_MODE_PA     a row is the key, then ceil(N / 8) bytes, column i = bit i & 7 of byte i >> 3
 * `rows` needs no alignment.  The padding bits of an input PA row never reach a result.  Keys are never read, only moved.
 * PARAMETERS:
 *   cols       a HOST array of M = n_out distinct input column indices, each < N, in any order: output column j is input column
 *              cols[j].  NULL is the identity and requires M = N.
 *   min_abund  a >= 1 (exactly 1 for PA input): a sample holds a row from this count upwards
 *   min_rec, max_rec
 *   out_mode   KMX_MODE_COUNT (only from COUNT) or KMX_MODE_PA
 *   flags      KMX_SELECT_ZERO_BELOW (COUNT output only)
 * PER ROW:
 *   present_j = (count[cols[j]] >= a) for COUNT, the bit of column cols[j] for PA
 *   rec       = the sum of present_j over j < M: the selected columns only
 * A row is KEPT iff min_rec <= rec <= max_rec.  min_rec > max_rec is valid and keeps nothing; max_rec >= M means no upper bound.
 * OUTPUT ROW: the key unchanged, then
 *   COUNT -> COUNT  M u32, v_j = count[cols[j]]; with KMX_SELECT_ZERO_BELOW v_j = 0 where v_j < a
 *   -> PA           ceil(M / 8) bytes, bit j & 7 of byte j >> 3 = present_j; the padding bits of the last byte are 0
 * OUTPUTS: the kept rows in the input's order (a valid body of the new row size); one kmx_select_rec per kept row in the same order; the
 * count of kept rows.
 * EXAMPLES.  N = 5, a row of counts (0, 3, 10, 1, 7), cols = (4, 2, 1):
 *   a = 3: present = (1, 1, 1), rec = 3, output counts (7, 10, 3)
 *   a = 5: present = (1, 1, 0), rec = 2, output counts (7, 10, 3); with KMX_SELECT_ZERO_BELOW (7, 10, 0); as PA the byte 0x03
 * The row (0, 0, 0, 9, 0) has rec 0: min_rec 1 drops it, min_rec 0 keeps it.
 * LIMITS, each refused before any GPU work.  KMX_E_INVAL: n_cols or n_out = 0; n_out > n_cols; a column index >= N or listed twice;
 * cols = NULL with M != N; key_words 0 or > 4; a mode or out_mode other than COUNT / PA; PA -> COUNT; min_abund 0; min_abund > 1 with PA
 * input; KMX_SELECT_ZERO_BELOW with PA output; unknown flag bits.  KMX_E_UNSUPPORTED: KMX_MODE_BF, KMX_MODE_BFC, KMX_MODE_BFT as the
 * input's mode (a Bloom row's identity is its position: rows cannot be dropped); n_rows > 2^32 - 256 (the placement tiles are the
 * filter's: 256 rows); a row of 4 GiB or more.
 * SCRATCH from the context's pool, per call: two 4-byte words per input row (keep, recurrence), the selection table (N bytes; PA:
 * ceil(N / 8)) and the column list (4 bytes a column) -- given back when the call has run; a 4-byte counter per 256 rows and the outputs,
 * sized for every row kept (n_rows * output row bytes + 16, and 8 * n_rows), live until the result is freed; for _host the uploaded rows.
 * Send a body that does not fit in runs of rows. */
#define KMX_SELECT_ZERO_BELOW 1u

typedef struct {
  uint32_t        key_words;     /* 1 ... 4 */
  uint32_t        mode;          /* KMX_MODE_COUNT | KMX_MODE_PA */
  uint32_t        n_cols;        /* N: samples of the matrix */
  uint32_t        n_out;         /* M: samples of the result */
  const void*     rows;
  uint64_t        n_rows;
  const uint32_t* cols;          /* HOST: M input column indices (copied by the call), or NULL: the identity */
  uint32_t        min_abund;     /* a */
  uint32_t        min_rec;
  uint32_t        max_rec;       /* >= M: no upper bound */
  uint32_t        out_mode;      /* KMX_MODE_COUNT | KMX_MODE_PA */
  uint32_t        flags;         /* KMX_SELECT_ZERO_BELOW */
  uint32_t        reserved;      /* 0 */
} kmx_select_task;               /* 64 bytes */

typedef struct {
  uint32_t row;          /* index in the input */
  uint32_t rec;
} kmx_select_rec;        /* 8 bytes */

typedef struct kmx_select_result kmx_select_result;

/* _dev and _host as for kmx_diff_*: rows a DEVICE pointer (a merge result's, a filter's, a combine's, a diff's or another select's body,
 * the caller's own memory), the kernels queued on the context's stream and the call back without waiting; or a HOST pointer, uploaded on
 * a stream of its own, the buffer free for reuse once _result_wait has returned.  cols is a host array in both. */
int kmx_select_dev(kmx_ctx* ctx, const kmx_select_task* task, kmx_select_result** out);
int kmx_select_host(kmx_ctx* ctx, const kmx_select_task* task, kmx_select_result** out);
int       kmx_select_result_wait(kmx_select_result* r);
/* (the accessors below wait for the call themselves) */
uint64_t  kmx_select_result_rows(kmx_select_result* r);                /* kept rows */
uint64_t  kmx_select_result_row_bytes(const kmx_select_result* r);     /* of an output row */
uint64_t  kmx_select_result_body_bytes(kmx_select_result* r);          /* rows * row_bytes */
const void*           kmx_select_result_body_dev(kmx_select_result* r);  /* the kept rows, in HBM until the result is freed */
int       kmx_select_result_copy_body(kmx_select_result* r, void* host_dst, uint64_t dst_bytes);
const kmx_select_rec* kmx_select_result_recs_dev(kmx_select_result* r);
int       kmx_select_result_copy_recs(kmx_select_result* r, kmx_select_rec* host_dst, uint64_t dst_entries);
double    kmx_select_result_kernel_ms(kmx_select_result* r);           /* needs kmx_set_profiling(ctx, 1); < 0 if unavailable */
/* algorithmic bytes: the body read once + the kept rows written at their new size + 8 bytes per kept row */
uint64_t  kmx_select_result_algo_bytes(kmx_select_result* r);
void      kmx_select_result_free(kmx_select_result* r);

/* -------------------------------------------------------------------- pan */

/* The recurrence spectrum of a matrix (what pangrowth and Panacus `hist` / `histgrowth` / `ordered-histgrowth` compute; no counterpart in
 * the kmtricks tree): how many rows are held by 0, 1, ... M of a list of samples, at which sample of the list a row is first met and
 * first missed, and per sample how many rows of each recurrence it holds.  The pangenome growth and core curves follow from the first
 * table in closed form, on the host.
 * INPUT, as for kmx_select_*: a run of n_rows rows of ONE partition's matrix body, n_cols = N samples:
 *   key_words 1 ... 4, KMX_MODE_COUNT  a row is 8 * key_words key bytes, then N u32 counts
 *   key_words 1 ... 4, KMX_MODE_PA     a row is the key, then ceil(N / 8) bytes, column i = bit i & 7 of byte i >> 3
 * `rows` needs no alignment.  The padding bits of a PA row never reach a result.  Keys are never read.
 * PARAMETERS:
 *   cols       select's convention: a HOST array of M = n_use distinct input column indices, each < N, in any order; NULL is the
 *              identity and requires M = N.  The list's ORDER is the order in which samples are "added" for the ordered curves:
 *              ordinal j is input column cols[j].
 *   min_abund  a >= 1 (exactly 1 for PA): a sample holds a row from this count upwards
 *   flags      KMX_PAN_SHARED
 * PER ROW:
 *   present_j = (count[cols[j]] >= a) for COUNT, the bit of column cols[j] for PA
 *   rec       = the sum of present_j over j < M
 *   first     = min{ j : present_j }, M if there is none
 *   gap       = min{ j : !present_j }, M if there is none
 * OUTPUTS: u64 DEVICE tables.  The call ADDS into a table of the caller's, or into a zeroed one the result owns when the pointer is
 * NULL.  Partitions and runs of rows accumulate in any order; n_rows = 0 adds nothing.
 *   spectrum[3][M + 1]   [0][r] the rows with rec = r; [1][j] the rows with first = j; [2][j] the rows with gap = j
 *   shared[M + 1][N]     (KMX_PAN_SHARED only) shared[r][c] the rows with rec = r in which INPUT column c is a listed column and
 *                        present.  Unlisted columns and row r = 0 stay untouched.  (Indexed by input column so that a wave's adds are
 *                        contiguous; a driver permutes for printing.)
 * EXAMPLE.  N = 4, cols NULL, a = 1, four rows:
 *   (1,0,2,0)  rec 2, first 0, gap 1
 *   (0,0,0,5)  rec 1, first 3, gap 0
 *   (3,3,3,3)  rec 4, first 0, gap 4
 *   (0,0,0,0)  rec 0, first 4, gap 0
 *   spectrum[0] = (1,1,1,0,1), spectrum[1] = (2,0,0,1,1), spectrum[2] = (2,1,0,0,1)
 *   shared[1] = (0,0,0,1), shared[2] = (1,0,1,0), shared[4] = (1,1,1,1), every other row of shared is zero
 * With a = 3 the first row has rec 0.  With cols = (3,0) the second row has rec 1, first 0, gap 1.
 * IDENTITIES of one call's increments: the sum of spectrum[0] is n_rows; spectrum[1][M] = spectrum[0][0]; spectrum[2][M] =
 * spectrum[0][M]; the sum of shared[r] over c is r * spectrum[0][r]; the sum of shared[.][c] over r is the number of rows that hold c
 * (with a = 1 inter[c][c] of kmx_dist_*, the presence tally of kmx_colsums_* on PA rows).
 * LIMITS, each refused before any GPU work.  KMX_E_INVAL: n_cols or n_use = 0; n_use > n_cols; a column index >= N or listed twice;
 * cols = NULL with M != N; key_words 0 or > 4; a mode other than COUNT / PA; min_abund 0; min_abund > 1 with PA; unknown flag bits; a
 * shared table without KMX_PAN_SHARED.  KMX_E_UNSUPPORTED: KMX_MODE_BF, KMX_MODE_BFC, KMX_MODE_BFT (a Bloom row is a hash bit: its
 * recurrence is not a k-mer's); n_rows > 2^32 - 256; a row of 4 GiB or more; KMX_PAN_SHARED with (M + 1) * N * 8 >= 8 GiB.
 * SCRATCH from the context's pool, per call, given back when the call has run: the ordinal table (4 bytes per input column, rounded up
 * to 8 columns), a call-local spectrum (24 * (M + 1) bytes); with KMX_PAN_SHARED 4 * (M + 1) bytes of class cursors and 12 bytes per
 * input row (its recurrence, and its (row, rec) place in recurrence order); for _host the uploaded rows.  The tables the result owns
 * (24 * (M + 1) bytes; with KMX_PAN_SHARED 8 * (M + 1) * N) live until the result is freed.  Send a body that does not fit in runs of
 * rows. */
#define KMX_PAN_SHARED 1u

typedef struct {
  uint32_t        key_words;     /* 1 ... 4 */
  uint32_t        mode;          /* KMX_MODE_COUNT | KMX_MODE_PA */
  uint32_t        n_cols;        /* N: samples of the matrix */
  uint32_t        n_use;         /* M: samples of the list */
  const void*     rows;
  uint64_t        n_rows;
  const uint32_t* cols;          /* HOST: M input column indices in the order they are added (copied by the call), or NULL: the identity */
  uint32_t        min_abund;     /* a */
  uint32_t        flags;         /* KMX_PAN_SHARED */
  uint64_t*       spectrum;      /* NULL, or a device table of 3 * (M + 1) u64 to accumulate into */
  uint64_t*       shared;        /* NULL, or (KMX_PAN_SHARED) a device table of (M + 1) * N u64 to accumulate into */
} kmx_pan_task;                  /* 64 bytes */

typedef struct kmx_pan_result kmx_pan_result;

/* _dev and _host as for kmx_select_*: rows a DEVICE pointer (a merge result's, a filter's, a combine's, a select's body, the caller's own
 * memory), the kernels queued on the context's stream and the call back without waiting; or a HOST pointer, uploaded on a stream of its
 * own, the buffer free for reuse once _result_wait has returned.  cols is a host array in both; spectrum and shared are device tables in
 * both and stay the caller's. */
int kmx_pan_dev(kmx_ctx* ctx, const kmx_pan_task* task, kmx_pan_result** out);
int kmx_pan_host(kmx_ctx* ctx, const kmx_pan_task* task, kmx_pan_result** out);
int       kmx_pan_result_wait(kmx_pan_result* r);
/* (the accessors below wait for the call themselves) */
uint64_t* kmx_pan_result_spectrum_dev(kmx_pan_result* r);      /* the table as it stands: the result's own or the task's */
uint64_t* kmx_pan_result_shared_dev(kmx_pan_result* r);        /* NULL without KMX_PAN_SHARED */
int       kmx_pan_result_copy_spectrum(kmx_pan_result* r, uint64_t* host_dst, uint64_t dst_entries);   /* 3 * (M + 1) entries */
int       kmx_pan_result_copy_shared(kmx_pan_result* r, uint64_t* host_dst, uint64_t dst_entries);     /* (M + 1) * N; KMX_E_INVAL without KMX_PAN_SHARED */
/* duration in ms of the call's kernels, the clearing of the tables the result owns included (needs kmx_set_profiling(ctx, 1)); < 0 if unavailable */
double    kmx_pan_result_kernel_ms(kmx_pan_result* r);
/* the same interval in its parts: clearing + k_pan_score + k_pan_fold, k_pan_order, k_pan_shared (the last two -1 without
 * KMX_PAN_SHARED); any pointer may be NULL */
int       kmx_pan_result_kernel_parts_ms(kmx_pan_result* r, double* score_ms, double* order_ms, double* shared_ms);
/* algorithmic bytes: the body read once (n_rows * row bytes) + the spectrum (24 * (M + 1)); with KMX_PAN_SHARED the body read once more,
 * 24 bytes per row (its recurrence and its place in the order, each written and read once) and the shared table (8 * (M + 1) * N)
 *  */
uint64_t  kmx_pan_result_algo_bytes(kmx_pan_result* r);
void      kmx_pan_result_free(kmx_pan_result* r);

/* ----------------------------------------------------------------- colors */

/* The distinct sample sets of a matrix's rows (the colour classes of a coloured de Bruijn graph -- Mantis, Bifrost, Fulgor and GGCAT store
 * k-mer -> class id plus a class table --, the exclusive regions of the N-way Venn diagram that an UpSet plot draws; no counterpart in
 * the kmtricks tree): which exact sets of samples occur as a row's presence pattern, how many rows each set has, and every row's set.
 * INPUT, as for kmx_pan_*: a run of n_rows rows of ONE partition's matrix body, n_cols = N samples:
 *   key_words 1 ... 4, KMX_MODE_COUNT  a row is 8 * key_words key bytes, then N u32 counts
 *   key_words 1 ... 4, KMX_MODE_PA     a row is the key, then ceil(N / 8) bytes, column i = bit i & 7 of byte i >> 3
 * `rows` needs no alignment.  The padding bits of a PA row never reach a result.  Keys are never read.
 * PARAMETERS:
 *   cols       pan's convention: a HOST array of M = n_use distinct input column indices, each < N, in the caller's order; NULL is the
 *              identity and requires M = N.  Ordinal j is input column cols[j].
 *   min_abund  a >= 1 (exactly 1 for PA): a sample holds a row from this count upwards
 *   flags      none is defined: 0
 * PER ROW:
 *   present_j = (count[cols[j]] >= a) for COUNT, the bit of column cols[j] for PA
 *   pattern   = the M-bit vector (present_0 ... present_{M-1}) packed as a PA payload of M columns in u64 words: ordinal j = bit j & 63
 *               of word j >> 6; W = ceil(M / 64) words; the unused high bits of the last word are zero
 * CLASSES: two rows are of one class exactly when their patterns are equal -- every word is compared, never a hash alone.  The classes
 * are numbered 0 ... C - 1 in the order of their first row: class c's first row comes before class c + 1's.  The all-zero pattern is a
 * class like any other.
 * OUTPUTS, device memory the result owns (the _copy_ accessors bring them to the host; all wait for the call themselves):
 *   n_classes       C
 *   ids[n_rows]     u32, the class of every row
 *   first[C]        u32, the class's first row
 *   size[C]         u32, its rows
 *   patterns[C][W]  u64
 * EXAMPLE.  N = 4, cols NULL, a = 1, six rows (1,0,2,0) (0,0,0,5) (3,0,1,0) (0,0,0,0) (0,0,0,1) (7,0,9,0):
 *   C = 3, patterns = (5, 8, 0), first = (0, 1, 3), size = (3, 2, 1), ids = (0,1,0,2,1,0)
 *   a = 2:            C = 5, patterns = (4, 8, 1, 0, 5), size = (1,1,1,2,1), ids = (0,1,2,3,3,4)
 *   cols = (2, 0):    C = 2, patterns = (3, 0), first = (0, 1), size = (3, 3), ids = (0,1,0,1,1,0)
 * IDENTITIES: the sum of size is n_rows; ids[first[c]] = c; first is strictly ascending; the row first[c] has pattern patterns[c]; the
 * sizes summed by popcount(pattern) are spectrum[0] of kmx_pan_* on the same task.
 * LIMITS, each refused before any GPU work.  KMX_E_INVAL: n_cols or n_use = 0; n_use > n_cols; a column index >= N or listed twice;
 * cols = NULL with M != N; key_words 0 or > 4; a mode other than COUNT / PA; min_abund 0; min_abund > 1 with PA; flag bits.
 * KMX_E_UNSUPPORTED: KMX_MODE_BF, KMX_MODE_BFC, KMX_MODE_BFT (a Bloom row is a hash bit: its sample set is not a k-mer's);
 * n_rows > 2^32 - 256 (0xFFFFFFFF is the table's "empty"); a row of 4 GiB or more; scratch and result together beyond the device's
 * memory.  n_rows = 0 is a valid call with C = 0.  (KMX_E_NOMEM: the pool could not give what the device has in principle.)
 * SCRATCH from the context's pool, per call, given back when the call has run: PER ROW 8 * W + 24 bytes (the packed pattern, its 64-bit
 * signature, the row's representative, and per representative the class's first row, its size and the first row's rank) plus the
 * table, 4 bytes a slot, T = the power of two >= 2 * n_rows slots: 8 to 16 bytes a row -- 8 * W + 40 bytes a row at the most; 4 bytes a
 * listed column; 4 bytes per 256 rows; for _host the uploaded rows.  The RESULT keeps 8 * W + 12 bytes per input row until it is freed
 * (ids, and first / size / patterns sized for C = n_rows: C is known on the device only).  Send a body that does not fit in runs of
 * rows and merge the class tables (as `kmx colors` does).
 * KMX_E_INTERNAL from _wait and every accessor: a row found no slot within T probes (never expected: the table is at most half full). */
typedef struct {
  uint32_t        key_words;     /* 1 ... 4 */
  uint32_t        mode;          /* KMX_MODE_COUNT | KMX_MODE_PA */
  uint32_t        n_cols;        /* N: samples of the matrix */
  uint32_t        n_use;         /* M: samples of the list */
  const void*     rows;
  uint64_t        n_rows;
  const uint32_t* cols;          /* HOST: M input column indices in the caller's order (copied by the call), or NULL: the identity */
  uint32_t        min_abund;     /* a */
  uint32_t        flags;         /* 0 */
} kmx_colors_task;               /* 48 bytes */

typedef struct kmx_colors_result kmx_colors_result;

/* _dev and _host as for kmx_pan_*: rows a DEVICE pointer, the kernels queued on the context's stream and the call back without waiting;
 * or a HOST pointer, uploaded on a stream of its own, the buffer free for reuse once _result_wait has returned.  cols is a host array
 * in both. */
int kmx_colors_dev(kmx_ctx* ctx, const kmx_colors_task* task, kmx_colors_result** out);
int kmx_colors_host(kmx_ctx* ctx, const kmx_colors_task* task, kmx_colors_result** out);
int       kmx_colors_result_wait(kmx_colors_result* r);
/* (the accessors below wait for the call themselves) */
uint64_t  kmx_colors_result_n_classes(kmx_colors_result* r);           /* C; 0 after an error */
const uint32_t* kmx_colors_result_ids_dev(kmx_colors_result* r);       /* n_rows u32 on the device; NULL after an error */
int       kmx_colors_result_copy_ids(kmx_colors_result* r, uint32_t* host_dst, uint64_t dst_entries);        /* n_rows entries */
int       kmx_colors_result_copy_first(kmx_colors_result* r, uint32_t* host_dst, uint64_t dst_entries);      /* C */
int       kmx_colors_result_copy_sizes(kmx_colors_result* r, uint32_t* host_dst, uint64_t dst_entries);      /* C */
int       kmx_colors_result_copy_patterns(kmx_colors_result* r, uint64_t* host_dst, uint64_t dst_entries);   /* C * W */
/* duration in ms of the call's kernels, the clearing of the table included (needs kmx_set_profiling(ctx, 1)); < 0 if unavailable */
double    kmx_colors_result_kernel_ms(kmx_colors_result* r);
/* the same interval in its parts: k_col_pack; clearing + k_col_claim; k_col_flag + scan + k_col_number + k_col_ids + k_col_gather; any
 * pointer may be NULL */
int       kmx_colors_result_kernel_parts_ms(kmx_colors_result* r, double* pack_ms, double* claim_ms, double* number_ms);
/* algorithmic bytes: the body read once (n_rows * row bytes) + the packed patterns and signatures written once and read once
 * (2 * n_rows * (8 * W + 8)) + ids (4 * n_rows) + the class table (C * (8 + 8 * W)) */
uint64_t  kmx_colors_result_algo_bytes(kmx_colors_result* r);
void      kmx_colors_result_free(kmx_colors_result* r);

/* ------------------------------------------------------------------- gram */

/* The recurrence-weighted co-presence table of a matrix's samples (the integer part of the EIGENSTRAT / smartpca Gram matrix, the
 * kinship matrix of a k-mer GWAS; no counterpart in the kmtricks tree): T[i][j] = the sum over the rows that hold samples i and j of a
 * weight that depends on the row's recurrence alone.  With p = rec / M and the weight 1 / (p (1 - p)) in fixed point, the centred and
 * scaled Gram matrix of the samples follows from T and the tables of kmx_pan_* on the host (`kmx pca`).
 * INPUT, as for kmx_pan_*: a run of n_rows rows of ONE partition's matrix body, n_cols = N samples:
 *   key_words 1 ... 4, KMX_MODE_COUNT  a row is 8 * key_words key bytes, then N u32 counts
 *   key_words 1 ... 4, KMX_MODE_PA     a row is the key, then ceil(N / 8) bytes, column i = bit i & 7 of byte i >> 3
 * `rows` needs no alignment.  The padding bits of a PA row never reach a result.  Keys are never read.
 * PARAMETERS:
 *   cols       pan's convention: a HOST array of M = n_use distinct input column indices, each < N, in any order; NULL is the identity
 *              and requires M = N.  (The order of the list has no bearing on the table: it is indexed by input column.)
 *   min_abund  a >= 1 (exactly 1 for PA): a sample holds a row from this count upwards
 *   weights    a HOST array of M + 1 u32: the weight of recurrence class 0 ... M (copied by the call)
 *   flags      none is defined: 0
 * PER ROW:
 *   present_c = (count[c] >= a) for COUNT, the bit of column c for PA, for every LISTED input column c
 *   rec       = the number of listed columns present
 * OUTPUT: table[N][N], u64, row-major, DEVICE memory, indexed by INPUT column.  For every pair of listed input columns i, j that are
 * both present in a row the call ADDS weights[rec] to table[i][j]: both triangles are written, and the diagonal cell table[i][i] gets
 * weights[rec] for every row that holds listed column i.  Cells with an unlisted i or j are never touched; rows of a class of weight 0
 * add nothing.  The call adds into a table of the caller's, or into a zeroed one the result owns when the pointer is NULL.  Sums are
 * modulo 2^64: keeping the sum of weights[rec_r] over all the rows added into one table below 2^64 is the caller's business (`kmx pca`
 * chooses its fixed point from the spectrum for that).  Partitions and runs of rows accumulate in any order; n_rows = 0 adds nothing.
 * EXAMPLE.  N = 3, cols NULL, a = 1, weights = (0, 6, 3, 0), five rows:
 *   (1,0,0)  rec 1, weight 6: T00 += 6
 *   (1,1,0)  rec 2, weight 3: T00, T01, T10, T11 += 3
 *   (1,1,1)  rec 3, weight 0: nothing
 *   (0,0,0)  rec 0, weight 0: nothing
 *   (0,1,1)  rec 2, weight 3: T11, T12, T21, T22 += 3
 *   table = ((9,3,0),(3,6,3),(0,3,3))
 * IDENTITIES of one call's increments: (a) table[i][i] = the sum over R of weights[R] * shared[R][i] of kmx_pan_* on the same task;
 * (b) with weights = (0,1,1,...,1) and a = 1 the table is inter of kmx_dist_* on the listed columns; (c) the sum of table[i][j] over
 * the listed j = the sum over R of R * weights[R] * shared[R][i].
 * LIMITS, each refused before any GPU work.  KMX_E_INVAL: n_cols or n_use = 0; n_use > n_cols; a column index >= N or listed twice;
 * cols = NULL with M != N; key_words 0 or > 4; a mode other than COUNT / PA; min_abund 0; min_abund > 1 with PA; flag bits; weights
 * NULL.  KMX_E_UNSUPPORTED: KMX_MODE_BF, KMX_MODE_BFC, KMX_MODE_BFT; n_rows > 2^32 - 256; a row of 4 GiB or more; N > 32768 (a table
 * would be 8 GiB and more: the limit of kmx_dist_*).
 * SCRATCH from the context's pool, per call, given back when the call has run; W = n_rows / 64 + min(M + 1, n_rows) bounds the 64-row
 * words of the recurrence order (every class of a weight other than 0 starts on a word): the bit slab, 8 * 64 * ceil(N / 64) * W bytes;
 * the order and the words' weights, 260 * W bytes; 4 bytes per input row (its recurrence); 16 * (M + 1) bytes of class counts, cursors
 * and weights; a byte per input column or payload byte; for _host the uploaded rows.  The table the result owns (8 * N * N bytes) lives
 * until the result is freed.  Send a body that does not fit in runs of rows. */
typedef struct {
  uint32_t        key_words;     /* 1 ... 4 */
  uint32_t        mode;          /* KMX_MODE_COUNT | KMX_MODE_PA */
  uint32_t        n_cols;        /* N: samples of the matrix */
  uint32_t        n_use;         /* M: samples of the list */
  const void*     rows;
  uint64_t        n_rows;
  const uint32_t* cols;          /* HOST: M input column indices (copied by the call), or NULL: the identity */
  const uint32_t* weights;       /* HOST: M + 1 class weights (copied by the call) */
  uint32_t        min_abund;     /* a */
  uint32_t        flags;         /* 0 */
  uint64_t*       table;         /* NULL, or a device table of N * N u64 to accumulate into */
} kmx_gram_task;                 /* 64 bytes */

typedef struct kmx_gram_result kmx_gram_result;

/* _dev and _host as for kmx_pan_*: rows a DEVICE pointer, the kernels queued on the context's stream and the call back without waiting;
 * or a HOST pointer, uploaded on a stream of its own, the buffer free for reuse once _result_wait has returned.  cols and weights are
 * host arrays in both; table is a device table in both and stays the caller's. */
int kmx_gram_dev(kmx_ctx* ctx, const kmx_gram_task* task, kmx_gram_result** out);
int kmx_gram_host(kmx_ctx* ctx, const kmx_gram_task* task, kmx_gram_result** out);
int       kmx_gram_result_wait(kmx_gram_result* r);
/* (the accessors below wait for the call themselves) */
uint64_t* kmx_gram_result_table_dev(kmx_gram_result* r);       /* the table as it stands: the result's own or the task's */
int       kmx_gram_result_copy_table(kmx_gram_result* r, uint64_t* host_dst, uint64_t dst_entries);     /* N * N entries */
/* duration in ms of the call's kernels, the clearing of the table the result owns included (needs kmx_set_profiling(ctx, 1)); < 0 if unavailable */
double    kmx_gram_result_kernel_ms(kmx_gram_result* r);
/* the same interval in its parts: clearing + k_gram_score + k_gram_fold, k_gram_order, k_gram_slab, k_gram_pairs; any pointer may be
 * NULL */
int       kmx_gram_result_kernel_parts_ms(kmx_gram_result* r, double* score_ms, double* order_ms, double* slab_ms, double* pairs_ms);
/* algorithmic bytes: the body read twice (2 * n_rows * row bytes) + 16 bytes per row (its recurrence and its place in the order, each
 * written and read once) + the slab written and read once (2 * 8 * 64 * ceil(N / 64) * Wu, Wu the words the order takes: the sum over
 * the classes of a weight other than 0 of ceil(rows of the class / 64)) + the table (8 * N * N) */
uint64_t  kmx_gram_result_algo_bytes(kmx_gram_result* r);
void      kmx_gram_result_free(kmx_gram_result* r);

/* ------------------------------------------------------------------ assoc */

/* The structure-corrected association test of a matrix's rows (what kmdiff, EIGENSTRAT and a k-mer GWAS run once the samples' principal
 * components are known; no counterpart in the kmtricks tree): a phenotype -- case/control or quantitative -- is regressed on each row's
 * presence pattern with the covariates in the model.  The covariates are projected out of both sides: with Q an orthonormal basis of the
 * covariates (intercept included), y~ the phenotype's residual and x a row's 0/1 pattern, the score statistic is
 * (M - q) (x.y~)^2 / (|y~|^2 (|x|^2 - |Q'x|^2)).  The caller gives y~ and Q's columns in fixed point, so the per-row sums are exact
 * integers and the statistic uses + - * / on doubles alone (`kmx assoc`).
 * INPUT, as for kmx_pan_* / kmx_gram_*: a run of n_rows rows of ONE partition's matrix body, n_cols = N samples:
 *   key_words 1 ... 4, KMX_MODE_COUNT  a row is 8 * key_words key bytes, then N u32 counts
 *   key_words 1 ... 4, KMX_MODE_PA     a row is the key, then ceil(N / 8) bytes, column i = bit i & 7 of byte i >> 3
 * `rows` needs no alignment.  The padding bits of a PA row never reach a result.  Keys are never read, only moved.
 * PARAMETERS:
 *   cols       pan's convention: a HOST array of M = n_use distinct input column indices, each < N, in any order; NULL is the identity
 *              and requires M = N
 *   min_abund  a >= 1 (exactly 1 for PA): a sample holds a row from this count upwards
 *   n_vec      V, 1 ... 32
 *   vecs       a HOST array of M * V int32_t, vecs[m * V + j] the value of vector j for the m-th listed sample (copied by the call).
 *              Vector 0 is the phenotype with the covariates projected out; vectors 1 ... V - 1 are an orthonormal basis of the
 *              covariates, intercept included.  The call does not check that meaning: the definition below is over the integers as given.
 *   frac_bits  F, 0 ... 62; sc = 2^-F
 *   gain       double, finite, > 0
 *   vmin       double, >= 0
 *   threshold  double, not NaN, >= 0; +inf keeps nothing
 *   min_rec, max_rec   u32
 *   flags      none is defined: 0
 * PER ROW:
 *   present_c = (count[c] >= a) for COUNT, the bit of column c for PA, for every LISTED input column c
 *   rec       = the number of listed columns present
 *   s_j (i64) = the sum over the present listed samples m of vecs[m][j]
 * and then in IEEE double with no fused multiply-add, the operations and their order exactly these:
 *   u    = (double)s_0 * sc
 *   h    = 0; for j = 1 ... V-1 in ascending order: a = (double)s_j * sc; h = h + a * a
 *   v    = (double)rec - h
 *   if v > vmin:  beta = u / v;  stat = (gain * (u * u)) / v
 *   else:         beta = 0;      stat = 0
 * A row is KEPT iff min_rec <= rec <= max_rec and stat >= threshold.
 * OUTPUTS, the shape of kmx_diff_*: the kept rows whole, in the input's order (a valid body of the same row size); one kmx_assoc_rec per
 * kept row in the same order; the count of kept rows.
 * EXAMPLE.  N = M = 4, cols NULL, a = 1, V = 2, F = 2, gain = 3, vmin = 0.25, vecs rows (-2, 2), (-2, 2), (2, 2), (2, 2) -- the
 * phenotype (0, 0, 1, 1) centred, and the intercept 1/2 each:
 *   row (0,0,1,1)  rec 2, s0 =  4, u = 1,   s1 = 4, h = 1,    v = 1            stat = 3, beta = 1
 *   row (1,1,1,1)  rec 4, s0 =  0, u = 0,   s1 = 8, h = 4,    v = 0 <= vmin    stat = 0, beta = 0
 *   row (1,0,1,0)  rec 2, s0 =  0, u = 0,   s1 = 4, h = 1,    v = 1            stat = 0, beta = 0
 *   row (0,0,0,1)  rec 1, s0 =  2, u = 0.5, s1 = 2, h = 0.25, v = 0.75         stat = 1, beta = the double nearest 2/3
 * With threshold 1.0 rows 0 and 3 are kept, in that order.
 * LIMITS, each refused before any GPU work.  KMX_E_INVAL: n_cols or n_use = 0; n_use > n_cols; a column index >= N or listed twice;
 * cols = NULL with M != N; key_words 0 or > 4; a mode other than COUNT / PA; min_abund 0; min_abund > 1 with PA; V = 0 or V > 32; vecs
 * NULL; F > 62; a vector whose sum of |entries| is 2^53 or more ((double)s_j must be exact); gain not finite or <= 0; vmin negative or
 * NaN; a NaN or negative threshold; flag bits.  KMX_E_UNSUPPORTED: KMX_MODE_BF, KMX_MODE_BFC, KMX_MODE_BFT; n_rows > 2^32 - 256 (the
 * placement tiles are the filter's: 256 rows); a row of 4 GiB or more.  n_rows = 0 yields nothing.
 * SCRATCH from the context's pool, per call: a 4-byte keep word and a 32-byte record slot per input row, a 4-byte counter per 256 rows,
 * 40 bytes of the call's scalars, the vector table (4 bytes x N rounded up to 8 x V rounded up to one of 1, 2, 4, 8, 12, 16, 24, 32) and a byte per input column or
 * payload byte -- all given back when the call has run; the outputs are sized for every row kept (n_rows * row bytes + 16, and 32 *
 * n_rows) and live until the result is freed; for the _host calls the uploaded rows.  Send a body that does not fit in runs of rows. */
typedef struct {
  uint32_t        key_words;     /* 1 ... 4 */
  uint32_t        mode;          /* KMX_MODE_COUNT | KMX_MODE_PA */
  uint32_t        n_cols;        /* N: samples of the matrix */
  uint32_t        n_use;         /* M: samples of the list */
  const void*     rows;
  uint64_t        n_rows;
  const uint32_t* cols;          /* HOST: M input column indices (copied by the call), or NULL: the identity */
  const int32_t*  vecs;          /* HOST: M * V entries, vecs[m * V + j] (copied by the call) */
  uint32_t        n_vec;         /* V: 1 ... 32 */
  uint32_t        frac_bits;     /* F: 0 ... 62 */
  uint32_t        min_abund;     /* a */
  uint32_t        flags;         /* 0 */
  double          gain;
  double          vmin;
  double          threshold;     /* a kept row has stat >= threshold */
  uint32_t        min_rec;       /* ... and min_rec <= rec <= max_rec */
  uint32_t        max_rec;
} kmx_assoc_task;                /* 96 bytes */

typedef struct {
  double   stat;
  double   beta;
  int64_t  s0;
  uint32_t rec;
  uint32_t row;          /* index in the input */
} kmx_assoc_rec;         /* 32 bytes */

typedef struct kmx_assoc_result kmx_assoc_result;

/* _dev and _host as for kmx_diff_*: rows a DEVICE pointer, the kernels queued on the context's stream and the call back without waiting;
 * or a HOST pointer, uploaded on a stream of its own, the buffer free for reuse once _result_wait has returned.  cols and vecs are host
 * arrays in both. */
int kmx_assoc_dev(kmx_ctx* ctx, const kmx_assoc_task* task, kmx_assoc_result** out);
int kmx_assoc_host(kmx_ctx* ctx, const kmx_assoc_task* task, kmx_assoc_result** out);
int       kmx_assoc_result_wait(kmx_assoc_result* r);
/* (the accessors below wait for the call themselves) */
uint64_t  kmx_assoc_result_rows(kmx_assoc_result* r);                /* kept rows */
uint64_t  kmx_assoc_result_row_bytes(const kmx_assoc_result* r);
uint64_t  kmx_assoc_result_body_bytes(kmx_assoc_result* r);          /* rows * row_bytes */
const void*          kmx_assoc_result_body_dev(kmx_assoc_result* r); /* the kept rows, in HBM until the result is freed */
int       kmx_assoc_result_copy_body(kmx_assoc_result* r, void* host_dst, uint64_t dst_bytes);
const kmx_assoc_rec* kmx_assoc_result_recs_dev(kmx_assoc_result* r);
int       kmx_assoc_result_copy_recs(kmx_assoc_result* r, kmx_assoc_rec* host_dst, uint64_t dst_entries);
double    kmx_assoc_result_kernel_ms(kmx_assoc_result* r);           /* needs kmx_set_profiling(ctx, 1); < 0 if unavailable */
/* algorithmic bytes: the body read once + the kept rows written + 32 bytes per kept row + the vectors (4 * N * V) */
uint64_t  kmx_assoc_result_algo_bytes(kmx_assoc_result* r);
void      kmx_assoc_result_free(kmx_assoc_result* r);

/* ---------------------------------------------------------------- unitigs */

/* The compacted de Bruijn graph of a set of k-mers (what MUSET asks of ggcat behind `kmat_tools filter`, what kmdiff does when it merges
 * its significant k-mers into contigs; no counterpart in the kmtricks tree): every k-mer's unitig, its place and strand in it, and the
 * unitigs' sequences.  This comment is the contract.
 * INPUT: keys[n][key_words] u64, low word first, as the key part of a matrix row; dense (stride 8 * key_words bytes), 8-byte aligned.
 * key_words = ceil(kmer_size / 32).  The keys are n DISTINCT CANONICAL k-mers in ANY order (the rows of several partitions one behind
 * the other are not sorted).  The encoding is the matrices' own: digit i (bits 2i, 2i + 1) is base k - 1 - i, A0 C1 T2 G3, the
 * complement is digit ^ 2.  Node v is keys[v]; x is its key read as a string.
 * SIDES: side 1 is the right end of x, side 0 the left end.  The four EXTENSIONS of side 1 are x[1:] + c, those of side 0 c + x[:-1].
 * An extension y is PRESENT when canonical(y) is a key, of node u say; y ENTERS u on side t: from side 1, t = 0 if y == key(u), else 1;
 * from side 0, t = 1 if y == key(u), else 0.
 * deg(v, s) = the number of present extensions, 0 ... 4: STRINGS are counted; self-loops and hairpins (u == v) count.  (Two extensions
 * of one side cannot be each other's reverse complement -- x[1:] + c == revcomp(x[1:] + d) forces c == d --, so a side's present
 * extensions are distinct nodes; both SIDES of a node may lead to one node.)
 * A node is PALINDROMIC when key == revcomp(key) (even k only).
 * cand(v, s) = (u, t) when deg(v, s) == 1, u != v and neither v nor u is palindromic; otherwise there is none.
 * link(v, s) = (u, t) iff cand(v, s) = (u, t) and cand(u, t) = (v, s).  So each side has at most one link, links are symmetric, and a
 * component of the link graph is a simple path or a simple cycle: one UNITIG.
 * TRAVEL: leaving v through side s along link (u, t) means entering u at t and leaving it through 1 - t.  Node u is read forward
 * (ori = 0) when it is left through side 1, and as its reverse complement (ori = 1) otherwise.
 * A PATH has two traversals, one from each end: the one taken is the traversal whose FIRST oriented k-mer is the smaller key (most
 * significant word first); the two are never equal unless the path is a single palindromic node.  A single node is read forward.
 * A CYCLE starts at its node with the smallest key, read forward, leaving through side 1; it is flagged circular.
 * SEQUENCE: a unitig of L nodes is L + k - 1 bases: the first oriented k-mer, then the last base of each following one; a cycle the
 * same way, linearised at its start node.  Unitigs are numbered 0 ... U - 1 by ascending index of their start node (pos 0).
 * OUTPUTS, device memory the result owns (the _copy_ accessors bring them to the host; all wait for the call themselves):
 *   n_unitigs       U
 *   unitig[n]       u32, the node's unitig          pos[n]  u32, its position in it          ori[n]  u8, 0 forward, 1 reverse complement
 *   start[U]        u32, the node at pos 0, strictly ascending       len[U]  u32, k-mers       circ[U]  u8, 1 for a cycle
 *   seq_off[U + 1]  u64, exclusive sums of len + k - 1
 *   seqs            seq_off[U] = n + U (k - 1) bytes of ACGT, made by the first accessor that asks for them (sized from U on the host)
 * EXAMPLE.  k = 5 (below the call's own limit: for the reader and the CPU restatement), keys (ATTGC, CAATG, CAGGA, CCTGC, CTGCA, TTGCA,
 * TGCAC) = (173, 267, 316, 365, 436, 692, 721):
 *   U = 3, seqs = CATTGCA, TCCTGCA, TGCAC; unitig = (0,0,1,1,1,0,2), pos = (1,0,0,1,2,2,0), ori = (0,1,1,0,0,0,0), start = (1,2,6),
 *   len = (3,3,1), circ = (0,0,0)
 *   keys (ACCTG, AGGTC, CCTGA, CTGAC, TGACC): U = 1, seq ACCTGACCT, pos = (0,4,1,2,3), ori = (0,1,0,0,0), circ = (1)
 * IDENTITIES: len sums to n; unitig[start[u]] = u; pos is a permutation of 0 ... len - 1 within each unitig; the k-mers of a unitig's
 * sequence are its nodes' oriented keys in pos order.
 * LIMITS, each refused before any GPU work.  KMX_E_INVAL: kmer_size outside 8 ... 127; key_words != ceil(kmer_size / 32); null keys with
 * n > 0; flag bits.  KMX_E_UNSUPPORTED: n > 2^31 - 2 (a state 2 v + s and the sentinel 0xFFFFFFFF must fit in u32).  n = 0 is a valid
 * call with U = 0.
 * DATA ERRORS, found on the device and returned as KMX_E_INVAL by _wait and every accessor, the message naming the cause: a key with bits
 * set from 2 k upwards; a key greater than its reverse complement; a key that occurs twice.  KMX_E_INTERNAL: a probe sequence ran T
 * slots or a cycle walk 2 n steps (never expected: the table is at most half full).
 * SCRATCH from the context's pool, per call, given back when the call has run: PER NODE 16 bytes of candidates and links, 64 of the two
 * state buffers of the ranking (2 states x 16 bytes x 2), 13 for the numbering, plus the table, 4 bytes a slot, T = the power of two
 * >= 2 n slots: 8 to 16 bytes a node -- 109 bytes a node at the most; 8 bytes per 256 nodes.  The RESULT keeps 8 * key_words + 26 bytes
 * per node until it is freed (its own copy of the keys, unitig, pos, ori, and start / len / circ / seq_off sized for U = n: U is known
 * on the device only), and n + U (k - 1) bytes of sequence once they are asked for. */
typedef struct {
  const uint64_t* keys;          /* n * key_words words */
  uint64_t        n;
  uint32_t        kmer_size;     /* k: 8 ... 127 */
  uint32_t        key_words;     /* ceil(k / 32) */
  uint32_t        flags;         /* 0 */
  uint32_t        reserved;      /* not read */
} kmx_unitigs_task;              /* 32 bytes */

typedef struct kmx_unitigs_result kmx_unitigs_result;

/* _dev: keys a DEVICE pointer, copied by the call on the context's stream (free for reuse once _result_wait has returned), the kernels
 * queued behind it and the call back without waiting.  _host: a HOST pointer, uploaded on a stream of its own. */
int kmx_unitigs_dev(kmx_ctx* ctx, const kmx_unitigs_task* task, kmx_unitigs_result** out);
int kmx_unitigs_host(kmx_ctx* ctx, const kmx_unitigs_task* task, kmx_unitigs_result** out);
int       kmx_unitigs_result_wait(kmx_unitigs_result* r);
/* (the accessors below wait for the call themselves; after a data error each returns that error, 0 or NULL) */
uint64_t  kmx_unitigs_result_n_unitigs(kmx_unitigs_result* r);           /* U */
const uint32_t* kmx_unitigs_result_unitig_dev(kmx_unitigs_result* r);    /* n u32 on the device: the `groups` of kmx_groupsum_dev */
int       kmx_unitigs_result_copy_unitig(kmx_unitigs_result* r, uint32_t* host_dst, uint64_t dst_entries);      /* n */
int       kmx_unitigs_result_copy_pos(kmx_unitigs_result* r, uint32_t* host_dst, uint64_t dst_entries);         /* n */
int       kmx_unitigs_result_copy_ori(kmx_unitigs_result* r, uint8_t* host_dst, uint64_t dst_entries);          /* n */
int       kmx_unitigs_result_copy_start(kmx_unitigs_result* r, uint32_t* host_dst, uint64_t dst_entries);       /* U */
int       kmx_unitigs_result_copy_len(kmx_unitigs_result* r, uint32_t* host_dst, uint64_t dst_entries);         /* U */
int       kmx_unitigs_result_copy_circ(kmx_unitigs_result* r, uint8_t* host_dst, uint64_t dst_entries);         /* U */
int       kmx_unitigs_result_copy_seq_off(kmx_unitigs_result* r, uint64_t* host_dst, uint64_t dst_entries);     /* U + 1 */
uint64_t  kmx_unitigs_result_seq_bytes(kmx_unitigs_result* r);           /* n + U (k - 1) */
int       kmx_unitigs_result_copy_seqs(kmx_unitigs_result* r, uint8_t* host_dst, uint64_t dst_bytes);           /* seq_bytes */
/* duration in ms of the call's kernels, the clearing of the table included (needs kmx_set_profiling(ctx, 1)); < 0 if unavailable */
double    kmx_unitigs_result_kernel_ms(kmx_unitigs_result* r);
/* the same interval in its parts: clearing + k_ug_table; k_ug_cand + k_ug_link; the rounds of k_ug_jump; k_ug_paths, k_ug_cycles and the
 * numbering; any pointer may be NULL */
int       kmx_unitigs_result_kernel_parts_ms(kmx_unitigs_result* r, double* table_ms, double* links_ms, double* rank_ms, double* finish_ms);
/* algorithmic bytes: the keys read and the table cleared and filled; 8 look-ups a node, each a slot and a key; candidates and links
 * written and read; per round of the ranking a state's tuple read twice and written once (48 bytes a state); the ends' keys and the
 * outputs */
uint64_t  kmx_unitigs_result_algo_bytes(kmx_unitigs_result* r);
void      kmx_unitigs_result_free(kmx_unitigs_result* r);

/* --------------------------------------------------------------- groupsum */

/* A group-by over one partition's matrix body (MUSET's `kmat_tools unitig` with the unitig ids of kmx_unitigs_* as labels; the class ids
 * of kmx_colors_* are labels as well; no counterpart in the kmtricks tree): per group and listed sample how many of the group's rows
 * hold the sample and the sum of their counts.
 * INPUT, as for kmx_pan_*: n_rows rows of ONE partition's body, n_cols = N samples, KMX_MODE_COUNT or KMX_MODE_PA, `rows` at any
 * address; cols / n_use = M and min_abund = a are pan's.  groups[n_rows] u32, a label per row, lives where `rows` lives (device memory
 * for _dev, host memory for _host).  A window of labels: g0 and n_groups = G.
 * TABLES the call ADDS to, DEVICE pointers in both calls; NULL: the result owns a zeroed one -- exactly as the hits / sums of
 * kmx_kquery_*, so that the partitions of a run accumulate:
 *   size[G]         u32
 *   present[G][M]   u32
 *   sums[G][M]      u64   KMX_MODE_COUNT with KMX_GROUPSUM_SUMS only
 * PER ROW with g = groups[row] in [g0, g0 + G): size[g - g0] += 1; for each ordinal j that is present (count[cols[j]] >= a, or the PA
 * bit of cols[j]): present[g - g0][j] += 1 and, with sums, sums[g - g0][j] += count[cols[j]].  Rows outside the window -- 0xFFFFFFFF
 * among them -- add nothing.  The padding bits of a PA row never reach a result.
 * EXAMPLE.  N = 3, COUNT, a = 1, rows (1,0,2) (0,0,5) (3,0,1) (4,4,4), groups (7, 8, 7, 0xFFFFFFFF), g0 = 7, G = 2:
 *   size = (2, 1), present = ((2,0,2), (0,0,1)), sums = ((4,0,3), (0,0,5))
 * LIMITS, each refused before any GPU work.  KMX_E_INVAL: pan's (n_cols or n_use = 0, n_use > n_cols, a column index >= N or listed
 * twice, cols = NULL with M != N, key_words 0 or > 4, a mode other than COUNT / PA, min_abund 0 or > 1 with PA, unknown flag bits);
 * n_groups = 0; KMX_GROUPSUM_SUMS or a sums table with KMX_MODE_PA; a sums table without KMX_GROUPSUM_SUMS; null groups with n_rows > 0;
 * g0 + n_groups > 2^32.  KMX_E_UNSUPPORTED: Bloom modes; n_rows > 2^32 - 256; a row of 4 GiB or more; G * M > 2^32 table entries.
 * n_rows = 0 is a valid call.  The tables the result owns take 4 G + 4 G M (+ 8 G M) bytes; scratch: 4 bytes a listed column, for _host
 * the uploaded rows and labels. */
#define KMX_GROUPSUM_SUMS 1u
typedef struct {
  uint32_t        key_words;     /* 1 ... 4 */
  uint32_t        mode;          /* KMX_MODE_COUNT | KMX_MODE_PA */
  uint32_t        n_cols;        /* N */
  uint32_t        n_use;         /* M */
  const void*     rows;
  uint64_t        n_rows;
  const uint32_t* cols;          /* HOST: M input column indices (copied by the call), or NULL: the identity */
  const uint32_t* groups;        /* n_rows labels, where rows lives */
  uint32_t        min_abund;     /* a */
  uint32_t        flags;         /* KMX_GROUPSUM_SUMS or 0 */
  uint32_t        g0;            /* the window's first label */
  uint32_t        n_groups;      /* G */
  uint32_t*       present;       /* DEVICE [G][M], added to, or NULL */
  uint64_t*       sums;          /* DEVICE [G][M], added to, or NULL */
  uint32_t*       size;          /* DEVICE [G], added to, or NULL */
} kmx_groupsum_task;             /* 88 bytes */

typedef struct kmx_groupsum_result kmx_groupsum_result;

int kmx_groupsum_dev(kmx_ctx* ctx, const kmx_groupsum_task* task, kmx_groupsum_result** out);
int kmx_groupsum_host(kmx_ctx* ctx, const kmx_groupsum_task* task, kmx_groupsum_result** out);
int       kmx_groupsum_result_wait(kmx_groupsum_result* r);
/* (the accessors below wait for the call themselves; the tables are the ones the call added to, its own or the caller's) */
uint32_t* kmx_groupsum_result_present_dev(kmx_groupsum_result* r);
uint64_t* kmx_groupsum_result_sums_dev(kmx_groupsum_result* r);          /* NULL without KMX_GROUPSUM_SUMS */
uint32_t* kmx_groupsum_result_size_dev(kmx_groupsum_result* r);
int       kmx_groupsum_result_copy_present(kmx_groupsum_result* r, uint32_t* host_dst, uint64_t dst_entries);   /* G * M */
int       kmx_groupsum_result_copy_sums(kmx_groupsum_result* r, uint64_t* host_dst, uint64_t dst_entries);      /* G * M */
int       kmx_groupsum_result_copy_size(kmx_groupsum_result* r, uint32_t* host_dst, uint64_t dst_entries);      /* G */
double    kmx_groupsum_result_kernel_ms(kmx_groupsum_result* r);         /* needs kmx_set_profiling(ctx, 1); < 0 if unavailable */
/* algorithmic bytes: the body and the labels read once (n_rows * (row bytes + 4)) + the tables (G * (4 + 4 M), + 8 G M with sums)
 *  */
uint64_t  kmx_groupsum_result_algo_bytes(kmx_groupsum_result* r);
void      kmx_groupsum_result_free(kmx_groupsum_result* r);

/* ------------------------------------------------------------------- kset */

/* A set of k-mers resident on a device: built once, used by many kmx_match_* calls (the significant k-mers of kmx_diff_* / kmx_assoc_*,
 * the k-mers of the unitigs of kmx_unitigs_*, the row keys of a run).  This comment is the contract.
 * INPUT: keys[n][key_words] u64, low word first; dense (stride 8 * key_words bytes), 8-byte aligned.  key_words = ceil(kmer_size / 32).
 * The encoding is the matrices' own, exactly as the unitigs section says: digit i (bits 2i, 2i + 1) is base k - 1 - i, A0 C1 T2 G3, the
 * complement is digit ^ 2.  The keys are CANONICAL k-mers in ANY order.  DUPLICATES ARE ALLOWED: the ID of a key is the least index at
 * which it occurs, n_distinct the number of ids (the indices v with id[v] == v).
 * The set keeps its own copy of the keys: the caller's are free for reuse once kmx_kset_wait has returned.
 * LIMITS, each refused before any GPU work.  KMX_E_INVAL: kmer_size outside 8 ... 127; key_words != ceil(kmer_size / 32); null keys with
 * n > 0; flag bits.  KMX_E_UNSUPPORTED: n > 2^31.  n = 0 is a valid, empty set.
 * DATA ERRORS, found on the device; kmx_kset_wait, every accessor and every kmx_match_* call on the set return them as KMX_E_INVAL, the
 * message naming the cause: a key with bits set from 2 k upwards; a key greater than its reverse complement.
 * MEMORY the set holds until it is freed: 8 * key_words bytes a key plus the table -- 8 bytes a slot, (tag << 32) | index, T = the power
 * of two >= 2 n slots: 16 to 32 bytes a key.  4 bytes a key of scratch while kmx_kset_copy_ids runs.
 * Free a set when the kmx_match_* results made from it have been waited for. */
typedef struct {
  const uint64_t* keys;          /* n * key_words words */
  uint64_t        n;
  uint32_t        kmer_size;     /* k: 8 ... 127 */
  uint32_t        key_words;     /* ceil(k / 32) */
  uint32_t        flags;         /* 0 */
  uint32_t        reserved;      /* not read */
} kmx_kset_task;                 /* 32 bytes */

typedef struct kmx_kset kmx_kset;

/* _dev: keys a DEVICE pointer, copied by the call on the context's stream, the kernels queued behind it and the call back without
 * waiting.  _host: a HOST pointer, uploaded on a stream of its own. */
int kmx_kset_dev(kmx_ctx* ctx, const kmx_kset_task* task, kmx_kset** out);
int kmx_kset_host(kmx_ctx* ctx, const kmx_kset_task* task, kmx_kset** out);
int       kmx_kset_wait(kmx_kset* s);
/* (the accessors below wait for the build themselves; after a data error each returns that error or 0) */
uint64_t  kmx_kset_n(kmx_kset* s);
uint64_t  kmx_kset_n_distinct(kmx_kset* s);
uint32_t  kmx_kset_kmer_size(kmx_kset* s);
int       kmx_kset_copy_ids(kmx_kset* s, uint32_t* host_dst, uint64_t dst_entries);      /* n: for every input index, the id of its key */
double    kmx_kset_kernel_ms(kmx_kset* s);      /* clearing the table + k_ks_build + the count of ids (needs kmx_set_profiling(ctx, 1)); < 0 if unavailable */
void      kmx_kset_free(kmx_kset* s);

/* ------------------------------------------------------------------ match */

/* Reads against a set: which reads hold the set's k-mers, how many, on which strand, over how much of the read, and how often each k-mer
 * occurs (kmdiff's map-back, the read fetch of a k-mer GWAS, back_to_sequences).  This comment is the contract.
 * For every read q and every position i with i + k <= len(q) whose k bases are all ACGT (either case), let x be the k-mer at i and c its
 * canonical form.
 *   n_kmers[q]  counts the position.
 *   When c is in the set, with id j:
 *     hits[q]   counts it;
 *     fwd[q]    counts it when x == c: the read shows the key itself (a palindrome counts as forward);
 *     the bases i ... i + k - 1 of q are COVERED;
 *     first[q]  is the least such i and last[q] the greatest, relative to the read's start; both 0xFFFFFFFF when there is none;
 *     occ[j]    counts it (KMX_MATCH_OCC).  Only ids are ever counted: a duplicate's later indices keep what they had.
 *   covered[q]  the number of bases of q that lie in at least one hit.
 *   ids[p]      (KMX_MATCH_IDS; u32, one per base of the call) j for the position p = offsets[q] + i of a hit, 0xFFFFFFFF everywhere else.
 * Every occurrence counts; a read without a valid k-mer is reported with zeros.  Every result is an integer that does not depend on
 * the order of the adds.
 * occ: NULL (with KMX_MATCH_OCC the result owns a zeroed table), or a DEVICE table of n u64 (n the set's) that the call ADDS to: the
 * batches of a set of reads accumulate on the device.
 * EXAMPLE.  k = 5 (below the call's own limit: for the reader and the CPU restatement), keys (TTGCA, ATTGC, TTGCA, TGCAC) = (692, 173,
 * 692, 721): ids = (0, 1, 0, 3), n_distinct = 3.  Reads (CATTGCAC, ttgcaNtgcaat, ACGT, GGGGGGG, TGCAC):
 *   recs (n_kmers, hits, fwd, covered, first, last) = (4,3,3,7,1,3), (3,3,1,11,0,7), (0,0,0,0,-,-), (3,0,0,0,-,-), (1,1,1,5,0,0)
 *   occ = (3, 2, 0, 2); the ids that are not 0xFFFFFFFF, batch position -> id: 1 -> 1, 2 -> 0, 3 -> 3, 8 -> 0, 14 -> 0, 15 -> 1, 31 -> 3
 * LIMITS, each refused before any GPU work: a null set or one of another context, flag bits, null reads, an occ table without
 * KMX_MATCH_OCC (KMX_E_INVAL); fewer than 2^31 reads and fewer than 2^32 bases a call (KMX_E_UNSUPPORTED).  n_seqs = 0 is valid.  A set
 * with a data error: that error.
 * Scratch from the context's pool: 8 bytes per 64 bases (the hit bits).  The result keeps 24 bytes a read, with KMX_MATCH_IDS 4 bytes a
 * base, with KMX_MATCH_OCC and no table of the caller's 8 bytes a key. */
#define KMX_MATCH_IDS 1u
#define KMX_MATCH_OCC 2u
typedef struct { uint32_t n_kmers, hits, fwd, covered, first, last; } kmx_match_rec;      /* 24 bytes */
typedef struct {
  const kmx_kset* set;
  const char*     bases;
  const uint64_t* offsets;       /* [n_seqs + 1], offsets[0] = 0 */
  uint64_t        n_seqs;
  uint32_t        flags;         /* KMX_MATCH_IDS | KMX_MATCH_OCC */
  uint32_t        reserved;      /* not read */
  uint64_t*       occ;           /* NULL, or (with KMX_MATCH_OCC) a DEVICE table of n u64 to accumulate into */
  uint64_t        reserved2;     /* not read */
} kmx_match_task;                /* 56 bytes */

typedef struct kmx_match_result kmx_match_result;

/* _dev: bases and offsets DEVICE pointers; _host: HOST pointers, uploaded on a stream of its own (free for reuse once _result_wait has
 * returned).  The same division as the query calls. */
int kmx_match_dev(kmx_ctx* ctx, const kmx_match_task* task, kmx_match_result** out);
int kmx_match_host(kmx_ctx* ctx, const kmx_match_task* task, kmx_match_result** out);
int       kmx_match_result_wait(kmx_match_result* r);
/* (the accessors below wait for the call themselves) */
uint64_t  kmx_match_result_n_seqs(const kmx_match_result* r);
uint64_t  kmx_match_result_n_bases(const kmx_match_result* r);
int       kmx_match_result_copy_recs(kmx_match_result* r, kmx_match_rec* host_dst, uint64_t dst_entries);      /* n_seqs */
int       kmx_match_result_copy_ids(kmx_match_result* r, uint32_t* host_dst, uint64_t dst_entries);            /* n_bases; KMX_E_INVAL without KMX_MATCH_IDS */
uint64_t* kmx_match_result_occ_dev(kmx_match_result* r);                                                       /* the table the call added to; NULL without KMX_MATCH_OCC */
int       kmx_match_result_copy_occ(kmx_match_result* r, uint64_t* host_dst, uint64_t dst_entries);            /* n: the table as it stands; KMX_E_INVAL without KMX_MATCH_OCC */
uint64_t  kmx_match_result_total_kmers(kmx_match_result* r);
uint64_t  kmx_match_result_total_hits(kmx_match_result* r);
double    kmx_match_result_kernel_ms(kmx_match_result* r);      /* needs kmx_set_profiling(ctx, 1); < 0 if unavailable */
/* the same interval in its parts: the clears + k_mt_probe; k_mt_cover + k_mt_last; either pointer may be NULL */
int       kmx_match_result_kernel_parts_ms(kmx_match_result* r, double* probe_ms, double* cover_ms);
/* algorithmic bytes: the bases + 8 per valid k-mer (its slot) + 8 * key_words per tag match (the key it is confirmed against) + the
 * records (24 * n_seqs) + n_bases / 8 of hit bits written and read (2 * 8 * ceil(n_bases / 64)) + with KMX_MATCH_IDS 4 * n_bases + with
 * KMX_MATCH_OCC 8 per hit */
uint64_t  kmx_match_result_algo_bytes(kmx_match_result* r);
void      kmx_match_result_free(kmx_match_result* r);

/* ---------------------------------------------------------------- spectra */

/* The abundance spectrum of every listed sample and the joint spectrum of pairs of samples (what KAT `hist` / `comp` and Merqury's
 * spectra-cn tabulate; no counterpart in the kmtricks tree): how many rows a sample holds with a count of 0, 1, 2, ..., and how many rows
 * hold a count of a in sample x and of b in sample y.  dist's sum of minima and colsums' totals are summaries of these tables.
 * INPUT, as for kmx_pan_*: a run of n_rows rows of ONE partition's matrix body, n_cols = N samples, KMX_MODE_COUNT or KMX_MODE_PA,
 * `rows` at any address.  The padding bits of a PA row never reach a result.  Keys are never read.
 * PARAMETERS:
 *   flags      KMX_SPECTRA_HIST | KMX_SPECTRA_JOINT, at least one
 *   cols       (HIST) select's convention: a HOST array of M = n_use distinct input column indices, each < N, in any order; NULL is the
 *              identity and requires M = N.  Ordinal j is input column cols[j].
 *   cap1       (HIST) C1 in 1 ... 65535: counts of C1 and more share the last bin
 *   pairs      (JOINT) a HOST array of 2 * P input column indices (x_0, y_0, x_1, y_1, ...), each < N; x = y and repeated pairs are allowed
 *   cap2       (JOINT) C2 in 1 ... 255
 * PER ROW, with v_c the count of input column c (COUNT) or its bit (PA):
 *   HIST   for every j < M, v = v_cols[j]:  hist[j][min(v, C1)] += 1, and if v >= C1 also hist[j][C1 + 1] += v
 *   JOINT  for every p < P:                 joint[p][min(v_x, C2)][min(v_y, C2)] += 1
 * OUTPUTS: u64 DEVICE tables.  The call ADDS into a table of the caller's, or into a zeroed one the result owns when the pointer is
 * NULL.  Partitions and runs of rows accumulate in any order; n_rows = 0 adds nothing.
 *   hist[M][C1 + 2]            [j][b] for b <= C1 the rows by (capped) count; [j][C1 + 1] the volume of the last bin, so that the sum
 *                              over b < C1 of b * hist[j][b], plus hist[j][C1 + 1], is the column's exact total
 *   joint[P][C2 + 1][C2 + 1]   [p][a][b] the rows with (capped) counts a in x_p and b in y_p
 * EXAMPLE.  N = 3, cols NULL, C1 = 2, pairs (0,1), (2,2), C2 = 2, four rows:
 *   (1,0,2)   (0,0,5)   (3,3,3)   (0,0,0)
 *   hist[0] = (2,1,1, 3)   hist[1] = (3,0,1, 3)   hist[2] = (1,0,3, 10)
 *   joint[0]: [0][0] = 2, [1][0] = 1, [2][2] = 1;  joint[1]: [0][0] = 1, [2][2] = 3; every other cell is zero
 * With cols = (2) hist is the one line (1,0,3, 10).
 * IDENTITIES of one call's increments: the sum of hist[j][0 ... C1] is n_rows; the total above is colsums' sum of the column; the sum of
 * hist[j][1 ... C1] is the rows that hold the column; the sum of joint[p] is n_rows, its row sums are x_p's histogram folded at C2 and
 * its column sums y_p's; joint of (x, x) is diagonal; while no count reaches C2 the sum of min(a, b) * joint[p][a][b] is mins[x][y] of
 * kmx_dist_*.
 * LIMITS, each refused before any GPU work.  KMX_E_INVAL: n_cols = 0; no flag or unknown flag bits; key_words 0 or > 4; a mode other than
 * COUNT / PA; HIST with n_use = 0, n_use > n_cols, a column index >= N or listed twice, cols = NULL with M != N, cap1 outside 1 ... 65535;
 * without HIST n_use != 0, cols != NULL or hist != NULL; JOINT with n_pairs = 0, pairs NULL, a pair index >= N, cap2 outside 1 ... 255;
 * without JOINT n_pairs != 0, pairs != NULL or joint != NULL.  KMX_E_UNSUPPORTED: KMX_MODE_BF, KMX_MODE_BFC, KMX_MODE_BFT (a Bloom row
 * is a hash bit: it has no count); n_rows > 2^32 - 256; a row of 4 GiB or more; a table of 8 GiB or more (M * (C1 + 2) or
 * P * (C2 + 1)^2 entries of 2^30 and more).
 * SCRATCH from the context's pool, per call: 4 bytes per input column (rounded up to 8 columns) with HIST, 8 bytes a pair with JOINT;
 * for _host the uploaded rows.  The tables the result owns live until the result is freed. */
#define KMX_SPECTRA_HIST  1u
#define KMX_SPECTRA_JOINT 2u

typedef struct {
  uint32_t        key_words;     /* 1 ... 4 */
  uint32_t        mode;          /* KMX_MODE_COUNT | KMX_MODE_PA */
  uint32_t        n_cols;        /* N: samples of the matrix */
  uint32_t        n_use;         /* M: samples of the list (HIST; 0 without) */
  const void*     rows;
  uint64_t        n_rows;
  const uint32_t* cols;          /* HOST: M input column indices (copied by the call), or NULL: the identity */
  const uint32_t* pairs;         /* HOST: 2 * P input column indices (copied by the call) */
  uint32_t        n_pairs;       /* P */
  uint32_t        cap1;          /* C1 (HIST) */
  uint32_t        cap2;          /* C2 (JOINT) */
  uint32_t        flags;         /* KMX_SPECTRA_HIST | KMX_SPECTRA_JOINT */
  uint64_t*       hist;          /* NULL, or (HIST) a device table of M * (C1 + 2) u64 to accumulate into */
  uint64_t*       joint;         /* NULL, or (JOINT) a device table of P * (C2 + 1)^2 u64 to accumulate into */
} kmx_spectra_task;              /* 80 bytes */

typedef struct kmx_spectra_result kmx_spectra_result;

/* _dev and _host as for kmx_pan_*: rows a DEVICE pointer, the kernels queued on the context's stream and the call back without waiting;
 * or a HOST pointer, uploaded on a stream of its own, the buffer free for reuse once _result_wait has returned.  cols and pairs are host
 * arrays in both; hist and joint are device tables in both and stay the caller's. */
int kmx_spectra_dev(kmx_ctx* ctx, const kmx_spectra_task* task, kmx_spectra_result** out);
int kmx_spectra_host(kmx_ctx* ctx, const kmx_spectra_task* task, kmx_spectra_result** out);
int       kmx_spectra_result_wait(kmx_spectra_result* r);
/* (the accessors below wait for the call themselves) */
uint64_t* kmx_spectra_result_hist_dev(kmx_spectra_result* r);       /* the table as it stands: the result's own or the task's; NULL without HIST */
uint64_t* kmx_spectra_result_joint_dev(kmx_spectra_result* r);      /* NULL without JOINT */
int       kmx_spectra_result_copy_hist(kmx_spectra_result* r, uint64_t* host_dst, uint64_t dst_entries);    /* M * (C1 + 2); KMX_E_INVAL without HIST */
int       kmx_spectra_result_copy_joint(kmx_spectra_result* r, uint64_t* host_dst, uint64_t dst_entries);   /* P * (C2 + 1)^2; KMX_E_INVAL without JOINT */
/* duration in ms of the call's kernels, the clearing of the tables the result owns included (needs kmx_set_profiling(ctx, 1)); < 0 if unavailable */
double    kmx_spectra_result_kernel_ms(kmx_spectra_result* r);
/* the same interval in its parts: clearing + the HIST kernel, the JOINT kernel (-1 for the part that was not asked for); any pointer may be NULL */
int       kmx_spectra_result_kernel_parts_ms(kmx_spectra_result* r, double* hist_ms, double* joint_ms);
/* algorithmic bytes.  HIST: the body read once (n_rows * row bytes) + the table, 8 * M * (C1 + 2).  JOINT: the pairs go in groups of G
 * consecutive pairs (G = min(16, floor(12288 / (C2 + 1)^2)) while C2 <= 109, else 16); U_g is the number of distinct columns of group g
 * and n_groups = ceil(P / G).  When 256 * max U_g <= row bytes the columns are gathered: n_rows * u * (the sum of U_g) with u = 4
 * (COUNT) or 1 (PA); otherwise the rows are streamed once a group: n_groups * n_rows * row bytes.  To that the table, 8 * P * (C2 + 1)^2.
 * With both flags the sum of the two. */
uint64_t  kmx_spectra_result_algo_bytes(kmx_spectra_result* r);
void      kmx_spectra_result_free(kmx_spectra_result* r);

/* ------------------------------------------------------------------ count */

/* superk: concatenated super-k-mer records [u8 n][2-bit nts] of one
 * (sample, partition) with the u32 block-size framing of skp.<p> removed
 * (io/superk_storage.hpp:215-225).  HOST pointers.  Output: ascending
 * canonical k-mers (key_words = ceil(k/32) words each) with
 * count >= hard_min, saturated to u32; buffers released with kmx_free.
 * 8 <= kmer_size <= 127: the reference's default KMER_LIST "32 64 96 128" (CMakeLists.txt:25-27; loop_executor.hpp:47-63 picks
 * the first entry above k, and that type's width bounds a record: 28 k-mers for k < 32, 60 below 64, 92 below 96, 124 beyond --
 * Sequence2SuperKmer.hpp:146).  A record that claims more is refused (KMX_E_INVAL), not decoded. */
int kmx_count_kmer(kmx_ctx* ctx, const uint8_t* superk, uint64_t len, uint32_t kmer_size,
                   uint32_t hard_min, uint64_t** keys, uint32_t** counts, uint64_t* n_out);
/* window hashes XXH64(words, 8*ceil(k/32), 0) % window + window * partition */
int kmx_count_hash(kmx_ctx* ctx, const uint8_t* superk, uint64_t len, uint32_t kmer_size,
                   uint64_t window, uint64_t partition, uint32_t hard_min,
                   uint64_t** hashes, uint32_t** counts, uint64_t* n_out);

/* Batched form (one call per sample instead of one per (sample, partition)): superk[p] / len[p] are the
 * n_parts partition streams of one sample; hash_mode != 0 selects window hashes with
 * partition_ids[p] as the window index of stream p.  keys / counts / n_out are arrays of n_parts
 * entries; every keys[p] and counts[p] is released with kmx_free. */
int kmx_count_batch(kmx_ctx* ctx, uint32_t n_parts, const uint8_t* const* superk, const uint64_t* len,
                    uint32_t kmer_size, int hash_mode, uint64_t window, const uint64_t* partition_ids,
                    uint32_t hard_min, uint64_t** keys, uint32_t** counts, uint64_t* n_out);

/* -------------------------------------------------------------- transpose */

/* out[c][r] = in[r][c], bits LSB-first in each byte; nrows, ncols multiples
 * of 8; in row stride ncols/8 bytes, out row stride nrows/8 bytes.  HOST pointers. */
int kmx_transpose_bits(kmx_ctx* ctx, const uint8_t* in, uint64_t nrows, uint64_t ncols, uint8_t* out);

/* ------------------------------------------------------ super-k-mer split */

/* Splits `n_seqs` reads (concatenated in `bases`, read i = bases[offsets[i] .. offsets[i+1]))
 * into super-k-mers and returns, per partition, the concatenated 2-bit records
 * (same bytes the reference buffers before block framing).  repart: u16[4^m]
 * minimizer -> partition table.  out_bytes[p] / out_len[p] / out_kmers[p] are
 * arrays of nb_parts entries; each out_bytes[p] is released with kmx_free.
 * 8 <= kmer_size <= 127, 4 <= minim_size <= 15.  From k = 64 on (Kmer<96> / Kmer<128>) the split, its statistics, the sampling pass
 * kmx_count_reads and kmx_count_reads_dev work as below that; kmx_count_reads_dev_multi (several samples a call) answers
 * KMX_E_UNSUPPORTED there. */
int kmx_superk_partition(kmx_ctx* ctx, const char* bases, const uint64_t* offsets, uint64_t n_seqs,
                         uint32_t kmer_size, uint32_t minim_size, const uint16_t* repart,
                         uint32_t nb_parts, uint8_t** out_bytes, uint64_t* out_len, uint64_t* out_kmers);

/* The statistics the reference keeps beside the split (gatb PartiInfo<5>): every array is optional (NULL = not wanted)
 * and is ADDED to, so that the batches of a sample -- or the samples of a cohort -- accumulate:
 *   part_counters  [nb_parts * KMX_PINFO_STRIDE]: per partition nb_kmers, nb_kxmers, then nbk_per_radix[x * 256 + radix]
 *                  for x = 0..4 (kx-mers of x + 1 k-mers; fill_partitions.hpp:67-102, PartiInfo.hpp:266-287 PartiInfoFile order)
 *   minim_superks / minim_kmers [4^m]: super-k-mers and k-mers per minimizer (incSuperKmer_per_minimBin)
 *   minim_kxmers   [4^m]: kx-mers per minimizer -- what the sampled repartition balances
 *                  (SampleRepart, gatb RepartitionAlgorithm.cpp:182-215; Repartitor::computeDistrib, PartiInfo.cpp:48-103)
 *   nb_superk      running total of super-k-mers (needs minim_superks) */
#define KMX_PINFO_STRIDE (2 + 5 * 256)
typedef struct {
  uint64_t* part_counters;
  uint64_t* minim_superks;
  uint64_t* minim_kmers;
  uint64_t* minim_kxmers;
  uint64_t  nb_superk;
} kmx_superk_stats;
/* kmx_superk_partition + statistics.  out_bytes == NULL (then out_len / out_kmers are ignored): statistics only,
 * nothing is packed -- the sampling pass of the repartition, where `repart` may be any table (all zeros). */
int kmx_superk_partition_stats(kmx_ctx* ctx, const char* bases, const uint64_t* offsets, uint64_t n_seqs,
                               uint32_t kmer_size, uint32_t minim_size, const uint16_t* repart,
                               uint32_t nb_parts, uint8_t** out_bytes, uint64_t* out_len, uint64_t* out_kmers,
                               kmx_superk_stats* stats);

/* The sampling pass of the sampled repartition (gatb RepartitionAlgorithm.cpp:182-215, 395-496): statistics
 * (normally minim_kxmers only) of the SHORTEST PREFIX of the reads that holds more than `budget` super-k-mers -- the
 * reference's bank iterator is cancelled by the super-k-mer that brings its count past the sample size and stops
 * before the next read.  n_used = reads in that prefix (n_seqs when the batch does not reach the budget),
 * n_superk = their super-k-mers. */
int kmx_superk_sample(kmx_ctx* ctx, const char* bases, const uint64_t* offsets, uint64_t n_seqs,
                      uint32_t kmer_size, uint32_t minim_size, uint64_t budget, kmx_superk_stats* stats,
                      uint64_t* n_used, uint64_t* n_superk);

/* One sample (or one batch of its reads) from reads to counts in ONE call: kmx_superk_partition[_stats] + kmx_count_batch
 * with the super-k-mer streams never leaving HBM (what SuperKTask + CountTask / HashCountTask do through the skp files,
 * task.hpp:255-320, 367-392, 447-481).  keys / counts / n_out / out_kmers: arrays of nb_parts entries as in kmx_count_batch
 * (partition p's window index is p in hash mode); superk_bytes / superk_len: NULL, or arrays that receive the streams as
 * kmx_superk_partition returns them (--keep-tmp); superk_info: NULL or 2 * nb_parts numbers, per partition what
 * SuperKStorageWriter::SaveInfoFile reports for its skp file (io/superk_storage.hpp:205-225, 328-340: k-mers since the last
 * full 32 KB block, bytes of the blocks flushed before it); stats: NULL or as in kmx_superk_partition_stats. */
int kmx_count_reads(kmx_ctx* ctx, const char* bases, const uint64_t* offsets, uint64_t n_seqs,
                    uint32_t kmer_size, uint32_t minim_size, const uint16_t* repart, uint32_t nb_parts,
                    int hash_mode, uint64_t window, uint32_t hard_min,
                    uint64_t** keys, uint32_t** counts, uint64_t* n_out, uint64_t* out_kmers,
                    uint8_t** superk_bytes, uint64_t* superk_len, uint64_t* superk_info, kmx_superk_stats* stats);

/* ---- count lists that stay in HBM between the count and the merge stage ------------------------------------------
 * The reference's CountTask writes counts/partition_<p>/<id>.kmer and its merge task reads them back
 * (task.hpp:367-392, 690-743), erasing them afterwards unless --keep-tmp (task.hpp:676-688).  On a GPU with 288 GB of
 * HBM the lists of a whole cohort fit: a kmx_store is an arena of device memory on one GPU that holds packed
 * (key, count) records -- exactly a .kmer file body, what kmx_merge_dev takes -- until the store is destroyed.
 * Thread-safe (the contexts of several host threads append to one store); limit_bytes = 0: 60 % of the device's
 * memory.  A store on another GPU than the counting context is filled with a peer copy over xGMI. */
typedef struct kmx_store kmx_store;
int      kmx_store_create(int device, uint64_t limit_bytes, kmx_store** out);
void     kmx_store_destroy(kmx_store* s);
uint64_t kmx_store_used(const kmx_store* s);
/* How a context on GPU from_device fills a store on GPU to_device: 1 = peer access between the two is enabled (asked for on first
 * use: hipDeviceCanAccessPeer + hipDeviceEnablePeerAccess) and the copy is one DMA over their xGMI link; 0 = the runtime stages it
 * through host memory; negative = KMX_E_INVAL.  `kmx pipeline --gpus G` asks for every pair when it creates its stores and prints
 * the outcome in its summary line. */
int      kmx_peer_access(int from_device, int to_device);
uint64_t kmx_store_limit(const kmx_store* s);

/* kmx_superk_stats without the host arithmetic: the device's own u32 tables of ONE call, copied (not added) into the
 * caller's buffers -- best pinned (kmx_alloc_pinned).  part_radix: [nb_parts][5][256] kx-mers of x + 1 k-mers per radix
 * (PartiInfoFile's nbk_per_radix; nb_kmers / nb_kxmers of a partition are sums over it); minim_superks / minim_kmers:
 * [4^m].  Any pointer may be NULL.  nb_superk: super-k-mers of the call. */
typedef struct {
  uint32_t* part_radix;
  uint32_t* minim_superks;
  uint32_t* minim_kmers;
  uint64_t  nb_superk;
  /* the per-minimizer records in SPARSE form instead (most of the 4^m minimizers never occur in a sample: 8 MB of tables for
   * ~10^5 entries at m = 10): minim_sparse != NULL (room for 3 * minim_sparse_cap u32; minim_superks / minim_kmers are then
   * ignored) receives minim_sparse_n triples {minimizer, super-k-mers, k-mers} in no particular order.  More minimizers
   * than minim_sparse_cap: KMX_E_INVAL (4^m entries always suffice). */
  uint32_t* minim_sparse;
  uint64_t  minim_sparse_cap;
  uint64_t  minim_sparse_n;
} kmx_superk_raw;

/* kmx_count_reads with the results left on the device: partition p's (key, count) records -- ascending, packed as a
 * .kmer body with 4-byte counts -- go to stores[p % n_stores] (the merge stage shards partitions round-robin over the
 * GPUs: the list already lies where it will be merged), lists[p] = {device pointer, records}.  stats (added to, u64)
 * or raw (copied, u32) or neither.  KMX_E_NOMEM when a store is full: the call's results are dropped, but a store is a bump arena
 * without rollback -- what the call had already placed in other stores stays consumed until kmx_store_destroy (the caller sends the
 * sample through count files: kmx_count_reads; `kmx pipeline` does).
 * With superk_bytes == NULL (here and in kmx_count_reads) no super-k-mer record stream is built at all: the k-mers are cut
 * straight from the batch's bases, the counts are the same (SuperKmerBinInfoFile's numbers still come back in superk_info:
 * they are computed from the records' sizes).  raw's buffers are filled when the call returns. */
int kmx_count_reads_dev(kmx_ctx* ctx, const char* bases, const uint64_t* offsets, uint64_t n_seqs,
                        uint32_t kmer_size, uint32_t minim_size, const uint16_t* repart, uint32_t nb_parts,
                        int hash_mode, uint64_t window, uint32_t hard_min,
                        kmx_store* const* stores, uint32_t n_stores, kmx_list* lists, uint64_t* out_kmers,
                        uint8_t** superk_bytes, uint64_t* superk_len, uint64_t* superk_info,
                        kmx_superk_stats* stats, kmx_superk_raw* raw);

/* The bases of a batch on their way to the device AHEAD of the call that counts them (no reference counterpart: the reference reads
 * its super-k-mer files while it counts, task.hpp:367-392).  The copy is queued on a stream of its own and runs beside the kernels
 * of the call before it -- two count workers that each upload and then compute fall into step and leave the GPU idle for the length
 * of every upload (a third of the count stage of 1000 x 5 Mbp).  bases: page-locked (kmx_alloc_pinned), unchanged until
 * the counting call that takes them has returned.  *dev_bases is what kmx_count_reads_dev / kmx_count_reads of the SAME context then
 * get as `bases` (with the same offsets as for the host copy); kmx_reads_release gives the device block back after that call (or
 * instead of it).  At most KMX_READS_AHEAD uploads per context are alive at a time (KMX_E_INVAL beyond). */
#define KMX_READS_AHEAD 4
int  kmx_reads_upload(kmx_ctx* ctx, const char* bases, uint64_t n_bytes, const char** dev_bases);
void kmx_reads_release(kmx_ctx* ctx, const char* dev_bases);

/* kmx_count_reads_dev for SEVERAL samples in one call (no reference counterpart: SuperKTask + CountTask run per sample,
 * task.hpp:250-392; a small sample -- 1 Mbp -- is a few dozen kernels of 5-150 us each and four host round trips, which one call
 * for several samples pays once).  bases[i] / offsets[i] / n_seqs[i]: sample i's reads as in kmx_count_reads.  Results are
 * sample-major: lists[i * nb_parts + p], out_kmers[i * nb_parts + p], superk_info[2 * (i * nb_parts + p)], raw[i] (every sample's
 * statistics in the same form -- all sparse or all dense -- or raw == NULL).  Partition p of every sample goes to
 * stores[p % n_stores]; a hash window's id is p.  n_samples * nb_parts <= 65535; not while the abundance histogram is on
 * (kmx_hist_reset: it is per call).  The same lists, numbers and tables as n_samples calls of kmx_count_reads_dev. */
int kmx_count_reads_dev_multi(kmx_ctx* ctx, uint32_t n_samples, const char* const* bases, const uint64_t* const* offsets,
                              const uint64_t* n_seqs, uint32_t kmer_size, uint32_t minim_size, const uint16_t* repart_table,
                              uint32_t nb_parts, int hash_mode, uint64_t window, uint32_t hard_min,
                              kmx_store* const* stores, uint32_t n_stores, kmx_list* lists, uint64_t* out_kmers,
                              uint64_t* superk_info, kmx_superk_raw* raw);
/* device memory (a list of a store, a result body) into host memory; blocks until it is there */
int kmx_copy_to_host(kmx_ctx* ctx, void* host_dst, const void* dev_src, uint64_t bytes);
/* ... without the wait: the copy is queued behind the context's earlier ones and runs back to back with them -- a writer that
 * brings a matrix body over in pieces keeps two in flight, so the link does not idle while it hands a piece on (0.6 ms per piece
 * otherwise: 0.4 s of the 2.0 s that 92 GB of matrices take).  host_dst: page-locked (kmx_alloc_pinned).
 * kmx_copy_wait(ctx, ticket) blocks until that copy (and every one queued before it) is in host memory and gives the ticket back;
 * at most KMX_COPIES_AHEAD tickets are out at a time (KMX_E_INVAL beyond). */
#define KMX_COPIES_AHEAD 8
int kmx_copy_to_host_async(kmx_ctx* ctx, void* host_dst, const void* dev_src, uint64_t bytes, uint32_t* ticket);
int kmx_copy_wait(kmx_ctx* ctx, uint32_t ticket);

/* The abundance histogram of a sample (`--hist`): the reference's KHist (histogram.hpp:35-68) is fed EVERY distinct k-mer /
 * hash of the sample with its count, before the hard-min filter (count_processor.hpp:61, 135), one clone per partition,
 * summed (histogram.hpp:113-136).  kmx_hist_reset zeroes the context's device histogram and turns accumulation on: every
 * kmx_count_kmer / _hash / _batch / _reads call after it adds its distinct keys (on the device, where the run lengths are).
 * kmx_hist_read waits for them and fills uniq_bins / total_bins (upper - lower + 1 entries each: keys with count c, and c times
 * that), oob[4] = {keys below lower, keys above upper, the sums of their counts: lower, upper} and sums[2] = {distinct keys,
 * sum of counts} -- the fields of HistFileHeader + the two vectors of a .hist file (io/hist_file.hpp:30-116).
 * lower <= upper <= 255 (the reference always builds KHist(id, k, 1, 255): task_scheduler.hpp:103).  kmx_hist_off stops it. */
int kmx_hist_reset(kmx_ctx* ctx);
int kmx_hist_read(kmx_ctx* ctx, uint32_t lower, uint32_t upper, uint64_t* uniq_bins, uint64_t* total_bins, uint64_t* oob, uint64_t* sums);
int kmx_hist_off(kmx_ctx* ctx);

void kmx_free(void* p);

#ifdef __cplusplus
}
#endif
#endif
