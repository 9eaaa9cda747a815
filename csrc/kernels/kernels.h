// Host-side launch API of the tensorframes_amd HIP kernel library (gfx950 / CDNA4).
//
// These functions are torch-free: raw device pointers + hipStream_t. Each one
// checks the shapes it is handed against what its grid assumes before it
// launches (a bad launch can fault the whole node).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>
#include <vector>

#include "../common.h"

namespace tfa {
namespace k {

constexpr int kMaxRank = 8;

void check_launch(const char* what);

// ------------------------------------------------------------ elementwise
enum class BinOp : int {
  ADD, SUB, MUL, DIV, FLOORDIV, FLOORMOD, TRUNCMOD, MAX, MIN, POW, SQDIFF,
  EQ, NE, LT, LE, GT, GE, LAND, LOR, ATAN2, DIVNONAN,
};
enum class UnOp : int {
  NEG, ABS, SQUARE, SQRT, RSQRT, EXP, LOG, LOG1P, EXPM1, RECIP, RELU, RELU6, ELU, SELU,
  SIGMOID, TANH, SOFTPLUS, SOFTSIGN, FLOOR, CEIL, ROUND, SIGN, SIN, COS, TAN, NOT, IDENTITY,
  ERF, ISNAN, ISINF, ISFINITE,
};

// Broadcast descriptor: output dims and per-operand element strides (0 on broadcast dims).
struct Bcast {
  int rank = 0;
  int64_t dims[kMaxRank];
  int64_t sa[kMaxRank];
  int64_t sb[kMaxRank];
  int64_t sc[kMaxRank];  // third operand (Select)
};

// out = op(a, b). mode: 0 same-shape contiguous, 1 b scalar, 2 a scalar,
// 3 row-broadcast (b is [inner], a is [n/inner, inner]), 4 general broadcast.
void binary(BinOp op, DType dt, const void* a, const void* b, void* out, int64_t n, int mode,
            int64_t inner, const Bcast* bc, hipStream_t s);
// out_dtype is BOOL for comparisons/logical ops.
void unary(UnOp op, DType dt, const void* x, void* y, int64_t n, hipStream_t s);
void cast(DType from, DType to, const void* x, void* y, int64_t n, hipStream_t s);
void select(DType dt, const void* cond, const void* a, const void* b, void* out, int64_t n,
            const Bcast& bc, hipStream_t s);
void fill(DType dt, void* out, int64_t n, double value, hipStream_t s);
void range(DType dt, void* out, int64_t n, double start, double delta, hipStream_t s);


// ------------------------------------------------------------ reductions
enum class RedOp : int { SUM, PROD, MIN, MAX, MEAN, ALL, ANY };
// x viewed as [outer, r, inner] -> y [outer, inner]. workspace: see reduce_workspace_bytes.
size_t reduce_workspace_bytes(DType dt, int64_t outer, int64_t r, int64_t inner);
void reduce(RedOp op, DType dt, const void* x, void* y, int64_t outer, int64_t r, int64_t inner,
            void* workspace, hipStream_t s);
// The kernels one reduce() launch takes: plain host code, no device. reduce()
// and reduce_workspace_bytes() switch on this (the routing is written once)
// and the tests read it to know which kernel a shape lands on.
enum class RedRoute : int {
  ROW_WAVE_VEC, ROW_WAVE, ROW_BLOCK, ROW_SPLIT, ROW_SPLIT_FOLD,
  COL, COL_VEC, COL_SPLIT, COL_VEC_SPLIT, COL_SPLIT_FOLD, COL_VEC_SPLIT_FOLD, COUNT
};
struct ReducePlan {
  RedRoute route;
  int64_t S = 1;               // slices of r (partial slabs); 1: the kernel writes y itself
  int64_t rows_per_split = 0;  // r elements per slice
  int64_t fold = 0;            // slabs left by the fold pass, 0: no fold pass
  int64_t col_blocks = 0;      // column path: 256-thread blocks across inner
  int vec = 1;                 // elements per 16-byte load (1: scalar loads)
};
const char* reduce_route_name(RedRoute r);
// aligned16: whether x is 16-byte aligned (the vector kernels need it)
ReducePlan reduce_route(DType dt, int64_t outer, int64_t r, int64_t inner, bool aligned16);
// arg-reduce over r of [outer, r, inner]; out int32 or int64
void argreduce(bool is_min, DType dt, DType out_dt, const void* x, void* y, int64_t outer,
               int64_t r, int64_t inner, hipStream_t s);
// softmax / log-softmax over the last dim of [rows, cols]
void softmax(DType dt, bool log, const void* x, void* y, int64_t rows, int64_t cols, hipStream_t s);
// top-k along the last dim of [rows, cols]: values (dt) + indices (int32), sorted descending
void topk(DType dt, const void* x, void* vals, int32_t* idx, int64_t rows, int64_t cols, int k,
          hipStream_t s);
// segmented reductions: rows of x [n, inner] with segment ids (sorted or not) into [nseg, inner]
// ---- one-shot all-reduce over IPC-mapped peer buffers (oneshot.hip)
constexpr int kOneShotMaxRanks = 8;
constexpr size_t kOneShotSlotBytes = 64 << 10;                     // largest payload
constexpr size_t kOneShotFlagOffset = 2 * kOneShotSlotBytes;       // 2 slots x 8 ranks u32
constexpr size_t kOneShotErrOffset = kOneShotFlagOffset + 2 * 8 * 4;  // timeout word
constexpr size_t kOneShotBufBytes = kOneShotErrOffset + 256;
struct OneShotPeers {
  void* buf[kOneShotMaxRanks];  // every rank's buffer, mapped into this process ([rank] = own)
};
// timeout_us bounds every flag wait (a missing peer sets the error word)
void oneshot_all_reduce(RedOp op, DType dt, const void* in, void* out, int64_t n, int rank, int world,
                        const OneShotPeers& p, uint32_t epoch, uint64_t timeout_us, hipStream_t s);
// fault injection: one wave that spins for `us` microseconds (at most 60 s) on
// the device's realtime counter, then exits; work queued behind it on `s`
// waits (a stalled peer / slow rank, for the collective timeout tests)
void device_stall(uint64_t us, hipStream_t s);

size_t unsorted_segment_workspace_bytes(RedOp op, DType dt, int64_t n, int64_t inner, int64_t nseg);
void unsorted_segment_reduce(RedOp op, DType dt, DType idt, const void* x, const void* ids,
                             void* y, int64_t n, int64_t inner, int64_t nseg, void* workspace,
                             hipStream_t s);
// The route of one unsorted_segment_reduce() call (host only, as reduce_route).
enum class UsegRoute : int { TINY_INT, SMALL_INT, PRIVATE, SORTED_PERM };
struct UsegPlan {
  UsegRoute route;
  int64_t B = 0;             // tiny_int / private: row blocks (partial slabs)
  int G = 0;                 // private: lanes that share one output element in the final pass
  int64_t tile = 0;          // private: columns per block
  int64_t rows_per_block = 0;
  int inner_pad = 0;         // sorted_perm: inner rounded up to a power of two, at most 64
  bool wide = false;         // sorted_perm: inner > 64
};
UsegPlan unsorted_segment_route(RedOp op, DType dt, int64_t n, int64_t inner, int64_t nseg);
// "tiny_int", "small_int", "private_g<G>", "sorted_perm_p<inner_pad>" ("sorted_perm_wide" for inner > 64)
std::string unsorted_segment_route_name(const UsegPlan& p);
// segmented reduce with CSR offsets over contiguous rows (deterministic)
void segment_reduce_csr(RedOp op, DType dt, const void* x, const int64_t* offsets, void* y,
                        int64_t nseg, int64_t inner, hipStream_t s);

// ------------------------------------------------------------ groupBy (groupby.hip)
// keys [n] -> ids [n] (group of each row, groups in ascending key order) and
// uniq (first nseg entries: the distinct keys, ascending); returns nseg
// (synchronises the stream once to read it).
size_t factorize_workspace_bytes(DType dt, int64_t n);
int64_t factorize(DType dt, const void* keys, int64_t n, int64_t* ids, void* uniq, void* workspace,
                  size_t workspace_size, hipStream_t s);
// per-row 64-bit key hash (accumulate: combine with the hash already in h)
void key_hash(DType dt, const void* keys, int64_t n, uint64_t* h, bool accumulate, hipStream_t s);
void hash_mod(const uint64_t* h, int64_t n, int64_t world, int64_t* dest, hipStream_t s);
// string keys as W big-endian words (sign-flipped) + length, column-major [W+1][n]
void string_words(const int64_t* offs, const uint8_t* data, int64_t n, int W, int64_t* out, hipStream_t s);
// bounded-width string keys: [2][n] int64 = (sign-flipped big-endian word 0,
// tag = length for keys <= 8 bytes, else 9 + 62-bit hash); string_verify sets
// flag[0] when a row's bytes differ from its group representative's
void string_key_hash(const int64_t* offs, const uint8_t* data, int64_t n, int64_t* out, hipStream_t s);
void string_verify(const int64_t* offs, const uint8_t* data, const int64_t* ids, const int64_t* rep, int64_t n,
                   int* flag, hipStream_t s);
uint64_t string_key_hash_host(const uint8_t* p, int64_t len);  // the same hash on the host
// rows idx of a string column: lens[g] = length of row idx[g]; gather_bytes
// copies them to out at new_offs (the exclusive scan of lens)
void string_lens(const int64_t* offs, const int64_t* idx, int64_t n, int64_t* lens, hipStream_t s);
void gather_bytes(const uint8_t* data, const int64_t* offs, const int64_t* idx, const int64_t* new_offs, int64_t n,
                  uint8_t* out, hipStream_t s);
// ids [n] in [0, nseg) -> rows ordered by segment (stable) perm [n] and CSR
// offsets [nseg + 1]; out-of-range ids are dropped
size_t segment_csr_workspace_bytes(int64_t n, int64_t nseg);
void segment_csr(DType idt, const void* ids, int64_t n, int64_t nseg, int64_t* perm, int64_t* offsets,
                 void* workspace, size_t workspace_size, hipStream_t s);
// segment g = rows perm[offsets[g] .. offsets[g+1]) of x [*, inner] -> y [nseg, inner] (deterministic)
void segment_reduce_perm(RedOp op, DType dt, const void* x, const int64_t* perm, const int64_t* offsets, void* y,
                         int64_t nseg, int64_t inner, hipStream_t s);
// rep[g] = the last row of group g (ids in [0, nseg)), as the host path picks it
void group_representatives(const int64_t* ids, int64_t n, int64_t nseg, int64_t* rep, hipStream_t s);
// idx[g * size + j] = perm[offs[g] + j]: row ids of G segments of one size
void segment_rows(const int64_t* perm, const int64_t* offs, int64_t G, int64_t size, int64_t* idx, hipStream_t s);
// dst row idx[j] = src row j (rows of row_bytes bytes)
void scatter_rows(int64_t row_bytes, const void* src, const int64_t* idx, void* dst, int64_t nidx, hipStream_t s);
// shuffle records: column c of a row occupies bytes [off[c], off[c] + row_bytes[c])
// of an R-byte record (off ascending, word-aligned slots when possible)
constexpr int kMaxPackCols = 16;
struct PackCols {
  int n = 0;
  int64_t row_bytes[kMaxPackCols];
  int64_t off[kMaxPackCols];
  const void* ptr[kMaxPackCols];
};
// out[j] = record of source row perm[j] (perm null: row j)
void pack_rows(const PackCols& pc, const int64_t* perm, int64_t nrows, int64_t record_bytes, void* out,
               hipStream_t s);
// column buffers pc.ptr[c] [nrows, row_bytes[c]] <- records
void unpack_rows(const PackCols& pc, const void* in, int64_t nrows, int64_t record_bytes, hipStream_t s);
// rows ordered by destination (stable): perm [n]; counts [world] rows per destination
size_t partition_workspace_bytes(int64_t n);
void partition_rows(const int64_t* dest, int64_t n, int64_t world, int64_t* perm, int64_t* counts, void* workspace,
                    size_t workspace_size, hipStream_t s);

// ------------------------------------------------------------ row compaction (compact.hip)
// Stable compaction of whole rows by a byte mask (non-zero keeps the row):
// compact_plan counts the kept rows per tile of compact_tile_rows() rows,
// scans the tile counts into the workspace and returns the total
// (synchronises the stream once to read it, like factorize); compact_gather
// then copies the kept rows of every column src.ptr[c] [n, src.row_bytes[c]]
// into dst.ptr[c] [total, row_bytes[c]] (the `off` fields are ignored) and,
// when `index` is not null, writes the kept row indices [total]. The mask
// must not change between the two calls.
int compact_tile_rows();
size_t compact_workspace_bytes(int64_t n);
int64_t compact_plan(const uint8_t* mask, int64_t n, void* workspace, size_t workspace_size, hipStream_t s);
void compact_gather(const PackCols& src, const PackCols& dst, const uint8_t* mask, int64_t n, int64_t total,
                    const void* workspace, int64_t* index, hipStream_t s);
// the single-block scan under compact_plan, for other plan / write kernels:
// offs[t] = sum of counts[0 .. t), *total = the sum of all (device pointers)
void compact_scan_counts(const int32_t* counts, int64_t ntiles, int64_t* offs, int64_t* total, hipStream_t s);

// ------------------------------------------------------------ zero-word packing (pack_words.hip)
// Packs a contiguous device buffer of rows x wpr 32-bit words into `packed`
// (pack_layout.h: header, 1-bit-per-word mask, the non-zero words), dropping
// only words whose bit pattern is 0x00000000. `packed` holds
// pack_words_max_bytes(rows, wpr) bytes (dense + mask + header: nothing can
// overflow) and is 64-byte aligned. Asynchronous on `s`; afterwards the first
// 8 bytes of `packed` hold the number of value words.
size_t pack_words_max_bytes(int64_t rows, int64_t wpr);
void pack_words(const void* src, int64_t rows, int64_t wpr, void* packed, hipStream_t s);

// ------------------------------------------------------------ sort (sort.hip)
// DataFrame.orderBy / sortWithinPartitions. Every sort key becomes one
// unsigned 64-bit word per row whose unsigned order is the key's order (bool /
// uint8: the value; signed ints: sign-extended, bit 63 flipped; floats: the
// IEEE bits at the type's width with every NaN the canonical quiet NaN and
// -0.0 as +0.0, negative values complemented, the others with the sign bit
// set, a float32 word in the low 32 bits; a descending key is complemented at
// its own width). Rows are ordered by the tuple of words; the sort is stable.
constexpr int kMaxSortKeys = 8;
struct SortKeys {
  int n = 0;
  DType dtype[kMaxSortKeys];
  const void* ptr[kMaxSortKeys];  // [rows] each, contiguous
  int descending[kMaxSortKeys];
};
// words [keys.n][n] (int64 bit patterns, word-major), every key in one launch
void sort_encode(const SortKeys& keys, int64_t n, int64_t* words, hipStream_t s);
int sort_tile_rows();  // radix::kTile
size_t sort_argsort_workspace_bytes(int W, int64_t n);
// perm[j] = source row of output row j under the (stable) order of the word
// tuples: LSD over the words, and inside a word only over the 8-bit digits
// that vary (one reduction finds them; the stream is synchronised once to
// read the W masks). Returns the radix passes run.
int sort_argsort(const int64_t* words, int W, int64_t n, int64_t* perm, void* workspace, size_t workspace_size,
                 hipStream_t s);
// dst.ptr[c] row j = src.ptr[c] row perm[j] for every column (rows of
// row_bytes[c] bytes, `off` ignored); perm values must lie in [0, n)
void permute_rows(const PackCols& src, const PackCols& dst, const int64_t* perm, int64_t n, hipStream_t s);
// the same gather with its own source row count: dst.ptr[c] row j (j < n_out)
// = src.ptr[c] row idx[j]; indices may repeat and must lie in [0, n_src)
void take_rows(const PackCols& src, const PackCols& dst, const int64_t* idx, int64_t n_out, int64_t n_src,
               hipStream_t s);
// out[i] = rows of the sorted order (perm) whose word tuple is < splitters[i]
// ([S][W], row-major), lexicographically as unsigned words
void sort_bounds(const int64_t* words, int W, int64_t n, const int64_t* perm, const int64_t* splitters, int64_t S,
                 int64_t* out, hipStream_t s);

// ------------------------------------------------------------ distinct rows (unique.hip)
// DataFrame.dropDuplicates / distinct: the first row of every run of equal
// word tuples in a sorted order. words [W][n] are sort_encode's, perm [n] is
// sort_argsort's stable order (null: the rows are in order already). Position
// i is a head when i == 0 or any word of row perm[i] differs from that word of
// row perm[i - 1]. unique_plan writes the head bits and the tile offsets into
// the workspace and returns the number of heads (synchronises the stream once
// to read it, like compact_plan); unique_write then stores perm[i] of every
// head, in order, into kept [total]. perm values must lie in [0, n).
int unique_tile_rows();
size_t unique_workspace_bytes(int64_t n);
int64_t unique_plan(const int64_t* words, int W, int64_t n, const int64_t* perm, void* workspace,
                    size_t workspace_size, hipStream_t s);
void unique_write(const int64_t* perm, int64_t n, int64_t total, const void* workspace, int64_t* kept,
                  hipStream_t s);

// ------------------------------------------------------------ pivot (pivot.hip)
// groupBy(keys).pivot(p).agg(...): the long table, one record per (key, pivot
// value) in ascending (keys..., pivot) order, spread to the wide one. offsets
// [G + 1] is the CSR of the G keys over the m records, pivot_words [m] the
// records' pivot sort words (ascending as unsigned words inside one key, each
// at most once), value_words [V] the words of the output columns in their
// order. Cell j * G + g of output a is src[a][r] of the record r of key g whose
// word is value_words[j], fill[a] (its low 4 bytes for 4-byte elements) where
// there is none: bit copies, every cell written exactly once.
constexpr int kMaxPivotValues = 1024;
struct PivotSpreadCols {
  int n = 0;
  uint32_t wide = 0;               // bit a: output a has 8-byte elements (else 4-byte)
  const void* src[kMaxPackCols];   // [m], contiguous
  void* dst[kMaxPackCols];         // [V][G]
  int64_t fill[kMaxPackCols];
};
int pivot_block_threads();
void pivot_spread(const int64_t* offsets, const int64_t* pivot_words, const int64_t* value_words, int64_t G, int64_t m,
                  int64_t V, const PivotSpreadCols& pc, hipStream_t s);

// ------------------------------------------------------------ join (join.hip)
// DataFrame.join: an equi-join of two frames on key tuples. Keys are the words
// of sort_encode (ascending), so equal words are Spark's key equality (NaN
// joins NaN, -0.0 joins 0.0). The build (right) side is sorted with
// sort_argsort and its words gathered into that order once:
// out[w][j] = words[w][perm[j]] (words, out: [W][m])
void join_gather_words(const int64_t* words, int W, int64_t m, const int64_t* perm, int64_t* out, hipStream_t s);
// per left row i (left: words [W][n]; right_sorted: [W][m], ascending tuples):
// lo[i] = sorted positions whose tuple is below row i's, cnt[i] = positions
// whose tuple equals it (they start at lo[i]); m == 0 gives zeros. mask_mode 1
// also writes mask[i] = (cnt[i] != 0), 2 writes mask[i] = (cnt[i] == 0), 0
// leaves mask alone
void join_probe(const int64_t* left, int W, int64_t n, const int64_t* right_sorted, int64_t m, int64_t* lo,
                int64_t* cnt, uint8_t* mask, int mask_mode, hipStream_t s);
// offs [n + 1] = exclusive scan of cnt [n] (offs[n] = the total, returned:
// the stream is synchronised once to read it); m bounds the counts
size_t join_scan_workspace_bytes(int64_t n);
int64_t join_scan(const int64_t* cnt, int64_t n, int64_t m, int64_t* offs, void* workspace, size_t workspace_size,
                  hipStream_t s);
// for every output row j in [0, total), with i the left row that has
// offs[i] <= j < offs[i + 1]: left_idx[j] = i, right_idx[j] =
// perm[lo[i] + (j - offs[i])]. A block owns join_tile_rows() output rows
int join_tile_rows();
void join_expand(const int64_t* offs, const int64_t* lo, const int64_t* perm, int64_t n, int64_t m, int64_t total,
                 int64_t* left_idx, int64_t* right_idx, hipStream_t s);

// ------------------------------------------------------------ stats (stats.hip)
// DataFrame.describe / summary / approxQuantile on device-resident columns.
// Columns are dense scalar columns [n] of uint8, int8, int16, int32, int64,
// float32 or float64 (mixed), read where they are: 16-byte vector loads from
// the first aligned element on, a scalar head and tail around them.
struct StatCols {
  int n = 0;
  DType dtype[kMaxPackCols];
  const void* ptr[kMaxPackCols];  // [rows] each, contiguous, aligned to the element
};
// one record per column in one launch pair: moments[c] = {n, mean, M2 (the sum
// of squared deviations from the mean)} as f64, every element converted to f64
// first; extremes[c] = {smallest, largest} order-preserving word of the column
// (the ascending table of the sort section). Welford per lane, Chan's merge
// across lanes, waves and (through per-block partial records and a one-block
// fold in block order) blocks: no float atomics, the same bits on every run.
// n == 0 launches nothing and leaves the outputs alone (the caller fills
// {0, NaN, NaN} and {all ones, 0}).
size_t column_moments_workspace_bytes(int ncols, int64_t n);
void column_moments(const StatCols& cols, int64_t n, double* moments, int64_t* extremes, void* workspace,
                    size_t workspace_size, hipStream_t s);
// one pair record per (xs[q], ys[q]) in one launch pair, for corr / covar_samp
// / covar_pop: records[q] = kPairRecordFields int64 bit patterns {n, mean_x,
// mean_y, M2_x, M2_y, C_xy = sum (x - mean_x)(y - mean_y)} as f64 (every
// element converted to f64 first) and the count of rows whose x or y is NaN or
// an infinity. The two columns of a pair may differ in dtype and alignment; a
// column may appear in several pairs. A lane takes runs of 16 consecutive rows
// (16-byte vector loads where a column's runs are aligned, scalar loads
// otherwise), the runs enter as batches, lanes, waves and blocks are merged in
// order with Chan's formula: no float atomics, the same bits on every run, a
// function of the row count alone. n == 0 launches nothing and leaves records
// alone (the caller fills zeros: the empty record).
constexpr int kPairRecordFields = 7;
size_t column_pair_moments_workspace_bytes(int npairs, int64_t n);
void column_pair_moments(const StatCols& xs, const StatCols& ys, int64_t n, int64_t* records, void* workspace,
                         size_t workspace_size, hipStream_t s);
// hist[p][d] (device int64 [P][256], overwritten) = rows whose word has its top
// prefix_bits bits (0, 8, ..., 56) equal to those of prefixes[p] (host) and whose
// next 8-bit digit is d; prefix_bits == 0 takes P == 1 and ignores the prefix.
// The word is computed from the raw column on the fly. 1 <= P <= kMaxPackCols.
// Per-wave LDS histograms, folded per block, added with 64-bit integer
// atomics: exact counts. A block reads tiles of stats_tile_rows() rows.
int stats_tile_rows();  // radix::kTile
void select_hist(DType dtype, const void* col, int64_t n, const int64_t* prefixes, int P, int prefix_bits,
                 int64_t* hist, hipStream_t s);

// ------------------------------------------------------------ grouped statistics (group_stats.hip)
// GroupedData.agg / DataFrame.agg. A record is kGroupRecordFields int64 bit
// patterns per (group, value column): n, mean, M2 (f64, every element
// converted to f64 first), the sum (a wrapping int64 sum for the integer
// dtypes, an f64 running sum for float32 / float64), the smallest and the
// largest ascending sort word. An empty record is {0, 0, 0, 0, all ones, 0}.
constexpr int kGroupRecordFields = 6;
int group_chunk_rows();  // rows per work item of group_moments
// records [nseg][cols.n][6] of the CSR segments (perm [nperm] row indices into
// the columns' n rows, offsets [nseg + 1]: segment_csr's result). A work item
// is at most group_chunk_rows() rows of one segment, taken by one wave
// (Welford per lane, Chan's merge in lane order); a segment's items are folded
// in chunk order. The chunk counts are scanned on the device and the stream
// is synchronised once to read their total. A record depends on the
// segment's rows in row order alone. n == 0 or nseg == 0 launches nothing.
// The work items are built by group_items (the chunk count and its scan, one
// stream synchronisation); a caller that needs both record kinds of one CSR
// builds them once and hands them to both passes (`items`), otherwise each
// pass builds its own in its workspace.
struct GroupItems {
  const int64_t* coffs = nullptr;  // device [nseg + 1]: the exclusive scan of the segments' chunk counts
  int64_t items = 0;               // coffs[nseg]
};
size_t group_items_workspace_bytes(int64_t nseg);
GroupItems group_items(const int64_t* offsets, int64_t nseg, int64_t nperm, void* workspace, size_t workspace_size,
                       hipStream_t s);
size_t group_moments_workspace_bytes(int ncols, int64_t nperm, int64_t nseg);
void group_moments(const StatCols& cols, int64_t n, const int64_t* perm, int64_t nperm, const int64_t* offsets,
                   int64_t nseg, int64_t* records, void* workspace, size_t workspace_size, hipStream_t s,
                   const GroupItems* items = nullptr);
// pair records [nseg][xs.n][kPairRecordFields] (the stats section) of the same
// CSR segments and work items: Welford per lane over rows gathered through
// perm, the lanes merged in lane order, a segment's chunks folded in chunk
// order. A record depends on the segment's rows in row order alone. n == 0
// or nseg == 0 launches nothing.
size_t group_pair_moments_workspace_bytes(int npairs, int64_t nperm, int64_t nseg);
void group_pair_moments(const StatCols& xs, const StatCols& ys, int64_t n, const int64_t* perm, int64_t nperm,
                        const int64_t* offsets, int64_t nseg, int64_t* records, void* workspace, size_t workspace_size,
                        hipStream_t s, const GroupItems* items = nullptr);
// out [ng][ncols][6] = records [m][ncols][6] rows offsets[g] .. offsets[g + 1]
// merged in order (Chan; integer sums add, float sums add in that order, words
// take min / max), starting from the group's first record. Bit c of
// float_mask: column c is float32 / float64
void merge_group_records(const int64_t* records, int64_t m, int ncols, uint32_t float_mask, const int64_t* offsets,
                         int64_t ng, int64_t* out, hipStream_t s);
enum class GroupStat : int { COUNT = 0, SUM, AVG, MIN, MAX, VAR_SAMP, VAR_POP, STDDEV_SAMP, STDDEV_POP };
struct GroupResultSpec {
  int n = 0;
  int col[kMaxPackCols];         // the record column an output reads
  GroupStat stat[kMaxPackCols];
  DType dtype[kMaxPackCols];     // that column's dtype
  void* out[kMaxPackCols];       // [ng]: int64 (COUNT, SUM of integers), the column's type (MIN, MAX), else f64
};
// every output column of merged records [ng][ncols][6] in one launch: words
// decoded to the column's type, describe's NaN / infinity rule (decided from
// the extreme words), the sample statistics NaN below two rows
void group_results(const int64_t* records, int64_t ng, int ncols, const GroupResultSpec& spec, hipStream_t s);
// out [ng][npairs][7] = pair records [m][npairs][7] rows offsets[g] ..
// offsets[g + 1] merged in order (Chan; the non-finite counts add), starting
// from the group's first record; a group without records gets the empty one
void merge_pair_records(const int64_t* records, int64_t m, int npairs, const int64_t* offsets, int64_t ng,
                        int64_t* out, hipStream_t s);
enum class PairStat : int { CORR = 0, COVAR_SAMP, COVAR_POP };
struct PairResultSpec {
  int n = 0;
  int pair[kMaxPackCols];  // the record pair an output reads
  PairStat stat[kMaxPackCols];
  double* out[kMaxPackCols];  // [ng]
};
// every output column of merged pair records [ng][npairs][7] in one launch:
// covar_pop = C / n (NaN without rows), covar_samp = C / (n - 1) (NaN below two
// rows), corr = C / sqrt(M2_x * M2_y) (NaN without rows or where an M2 is 0;
// not clamped); all three NaN where the record counts a non-finite row
void pair_results(const int64_t* records, int64_t ng, int npairs, const PairResultSpec& spec, hipStream_t s);

// ------------------------------------------------------------ window functions (window_scan.hip)
// Window / .over(). The n rows of one partition are sorted by (partition
// keys, order keys) and come as sort_encode's words [W][n]. A row is a group
// head when one of its first P words differs from the previous row's, a peer
// head when one of the W words does; row 0 is both (P == 0: one group). A
// channel is a segmented inclusive scan over the rows of a group, 8 bytes per
// row:
//   GROUP_HEAD / PEER_HEAD  the index of the row's group / peer head,
//   PEER_COUNT              peer heads of the group up to the row (dense_rank),
//   SUM_I64 / SUM_F64       the wrapping int64 / the f64 sum of a value column
//                           (every element converted first),
//   MIN_WORD / MAX_WORD     the smallest / largest ascending word of a column.
// In reverse the scan runs over the mirrored rows: a head is a row that
// differs from the next one, the two index channels give the last row of the
// row's group / peer run, the others scan from the group's end.
enum class WindowChan : int { GROUP_HEAD = 0, PEER_HEAD, PEER_COUNT, SUM_I64, SUM_F64, MIN_WORD, MAX_WORD };
struct WindowChans {
  int n = 0;
  int kind[kMaxPackCols];          // WindowChan
  DType dtype[kMaxPackCols];       // of the value column (SUM_I64 on)
  const void* ptr[kMaxPackCols];   // [n], contiguous, aligned to the element (SUM_I64 on)
};
int window_tile_rows();  // rows per tile of window_scan
// the operator a channel kind folds with: 0 wrapping int64 add, 1 f64 add, 2 / 3 unsigned min / max
int window_chan_op(int kind);
size_t window_scan_workspace_bytes(int nchan, int64_t n);
// out [ch.n][n] (int64 bit patterns). Reduce-then-scan in three launches (tile
// aggregates, one block over them, every tile again), no block waits for
// another; the order of the additions depends on n and window_tile_rows()
// alone. n == 0 launches nothing.
void window_scan(const int64_t* words, int W, int P, int64_t n, bool reverse, const WindowChans& ch, int64_t* out,
                 void* workspace, size_t workspace_size, hipStream_t s);
enum class WindowFn : int { ROW_NUMBER = 0, RANK, DENSE_RANK, COUNT, SUM, AVG, MIN, MAX };
enum class WindowFrame : int { ROWS = 0, RANGE, WHOLE };  // ..currentRow by rows, by peers; the whole group
struct WindowFinishSpec {
  int n_out = 0;
  WindowFn fn[kMaxPackCols];
  WindowFrame frame[kMaxPackCols];
  int chan[kMaxPackCols];        // the forward channel an output reads (DENSE_RANK, SUM, AVG, MIN, MAX)
  DType dtype[kMaxPackCols];     // the value column's dtype (MIN, MAX decode to it)
  void* out[kMaxPackCols];       // [n]: int32 (ranks), int64 (COUNT, SUM of SUM_I64), f64 (SUM of SUM_F64, AVG), the column's type
  int n_chan = 0;
  int op[kMaxPackCols];          // window_chan_op of every forward channel
  uint64_t carry[kMaxPackCols];  // the fold of the first group's pieces in earlier partitions
  uint64_t total[kMaxPackCols];  // the fold of all pieces of the last group
  int has_carry = 0, has_total = 0;     // the first group began earlier / the last group runs on
  int64_t carry_rows = 0, total_rows = 0;
};
// fwd [n_chan][n]: a forward window_scan whose channels 0 and 1 are GROUP_HEAD
// and PEER_HEAD; rev [2][n]: a reverse scan of those two. One elementwise
// launch: the carry applied (carry (+) value) to the rows of the first group,
// the value taken at the row (ROWS), its last peer (RANGE) or the group's last
// row (WHOLE; the total when the group runs on), decoded to the output column.
void window_finish(const int64_t* fwd, const int64_t* rev, int64_t n, const WindowFinishSpec& spec, hipStream_t s);

// ------------------------------------------------------------ holistic aggregates (group_order.hip)
// median / percentile, percentile_approx, mode and countDistinct per group.
// The n rows of one partition are sorted by (group keys, value columns) and
// come as sort_encode's words [W][n]; the first P words define the groups, all
// W the peer runs, the last word is the value. starts [ng + 1] lists the
// group heads in order (unique_plan / unique_write over the first P words),
// starts[ng] == n.
int group_order_chunk_rows();  // rows per work item of group_order_summary
size_t group_order_summary_workspace_bytes(int64_t n, int64_t ng);
// per group: distinct = its peer heads, mode_len = the length of its longest
// peer run and mode_pos that run's head row (among equal lengths the first).
// window_scan's PEER_HEAD channel, then a work item is at most
// group_order_chunk_rows() rows of one group, taken by one wave; a group's
// items are folded by a second kernel. Integers only; group_items
// synchronises the stream once. n < 2^31. n == 0 or ng == 0 launches nothing.
void group_order_summary(const int64_t* words, int W, int P, int64_t n, const int64_t* starts, int64_t ng,
                         int64_t* distinct, int64_t* mode_pos, int64_t* mode_len, void* workspace,
                         size_t workspace_size, hipStream_t s);
constexpr int kMaxPercentages = 16;
enum class GroupOrderFn : int { COUNT_DISTINCT = 0, MODE, PERCENTILE_APPROX, PERCENTILE };
struct GroupOrderSpec {
  int n_out = 0;
  GroupOrderFn fn[kMaxPackCols];
  int nq[kMaxPackCols];                        // percentages of the output (1 for the others)
  double pct[kMaxPackCols][kMaxPercentages];   // each in [0, 1]
  void* out[kMaxPackCols];  // [ng] int64 (COUNT_DISTINCT), [ng] of dtype (MODE), [ng][nq] of dtype / of f64
  DType dtype = DType::F32;  // of the value column
};
// one launch for all outputs. With N the rows of a group: PERCENTILE_APPROX is
// the word at rank max(ceil(p N) - 1, 0); PERCENTILE is, with pos = p (N - 1),
// lo = floor(pos), hi = ceil(pos), v_lo if lo == hi and otherwise
// (hi - pos) v_lo + (pos - lo) v_hi in f64 without contraction (a NaN leaves as
// the quiet NaN). value_words [n]: the last word of every row.
void group_order_finish(const int64_t* value_words, int64_t n, const int64_t* starts, const int64_t* distinct,
                        const int64_t* mode_pos, int64_t ng, const GroupOrderSpec& spec, hipStream_t s);

// ------------------------------------------------------------ random draws (random.hip)
// DataFrame.sample / randomSplit / sampleBy, F.rand / F.randn. Row i of a call
// draws from Philox4x32-10 with the key (seed low, seed high) and the counter
// (row low, row high, purpose, 0), row = row0 + i (64-bit), purpose 0 uniform,
// 1 normal, 2 poisson; the four words w0..w3 of one call serve one row:
//   u  = (((w0 << 32) | w1) >> 11) * 2^-53                         (exact)
//   z  = sqrt(-2 ln u1) * cospi(2 u2), u1 = (bits53(w0, w1) + 1) * 2^-53,
//        u2 = bits53(w2, w3) * 2^-53
// n == 0 launches nothing; outputs are [n], contiguous.
constexpr int kMaxStrata = 4096;       // sampleBy table entries (64 KiB of LDS)
constexpr int kMaxPoissonTable = 64;   // entries of a Poisson cdf table
int random_tile_rows();  // rows per block
void random_uniform(uint64_t seed, uint64_t row0, int64_t n, double* out, hipStream_t s);
void random_normal(uint64_t seed, uint64_t row0, int64_t n, double* out, hipStream_t s);
// mask[i] = (lo <= u_i && u_i < hi), one byte per row (compact_rows' mask)
void random_mask(uint64_t seed, uint64_t row0, int64_t n, double lo, double hi, uint8_t* mask, hipStream_t s);
// mask[i] = u_i < table_fractions[t] where table_words[t] == words[i], 0 when
// no entry does. words [n] are sort_encode's (one key); table_words [strata]
// ascending as unsigned words and distinct, 1 <= strata <= kMaxStrata
void random_mask_by(uint64_t seed, uint64_t row0, int64_t n, const int64_t* words, const int64_t* table_words,
                    const double* table_fractions, int strata, uint8_t* mask, hipStream_t s);
// counts[i] = entries of cdf [len] (non-decreasing, 1 <= len <= kMaxPoissonTable)
// that are <= u_i, u drawn under purpose 2
void random_poisson(uint64_t seed, uint64_t row0, int64_t n, const double* cdf, int len, int64_t* counts,
                    hipStream_t s);
// offs [n + 1] = the exclusive scan of counts (join_scan; offs[n] == total):
// idx [total] holds row i offs[i + 1] - offs[i] times, rows in order
void random_expand(const int64_t* offs, int64_t n, int64_t total, int64_t* idx, hipStream_t s);

// ------------------------------------------------------------ data movement
// dst[idx] = src[idx] over `dims`, both operands addressed by element strides
// (src strides may be 0 or negative; pointers already include the offsets).
constexpr int kMaxCopyPieces = 32;
struct CopyPieces {
  const void* src[kMaxCopyPieces];
  int64_t dst_off[kMaxCopyPieces];
  int64_t bytes[kMaxCopyPieces];
  int n = 0;
};
void batched_copy(const CopyPieces& pc, void* dst, hipStream_t s);
void strided_copy(int64_t elem_size, int rank, const int64_t* dims, const void* src,
                  const int64_t* src_strides, void* dst, const int64_t* dst_strides,
                  hipStream_t s);
// Gather rows: out[o, j, i] = params[o, idx[j], i]
void gather(int64_t elem_size, DType idt, const void* params, const void* idx, void* out,
            int64_t outer, int64_t axis_dim, int64_t nidx, int64_t inner, hipStream_t s);
void one_hot(DType dt, DType idt, const void* idx, void* out, int64_t n, int64_t depth,
             double on, double off, hipStream_t s);

// ------------------------------------------------------------ GEMM (MFMA)
// GEMM/conv epilogue activations (planner-fused unary op after the product
// and its bias); the formulas match the standalone elementwise kernels
enum Act : int { ACT_NONE = 0, ACT_RELU = 1, ACT_RELU6 = 2, ACT_SIGMOID = 3, ACT_TANH = 4, ACT_ELU = 5,
                 ACT_SELU = 6, ACT_SOFTPLUS = 7 };

// Elementwise chain absorbed into the GEMM/conv epilogue: after bias and
// activation, v = op_k(v, x_k) for k < n, where x_k is a scalar, a per-column
// [N] vector, a per-row [M] vector or a full [batch, M, N] tensor (the
// planner's match of ops that follow the product; formulas as the
// standalone elementwise kernels)
enum EpiCode : int { EPI_ADD = 0, EPI_SUB, EPI_RSUB, EPI_MUL, EPI_DIV, EPI_RDIV, EPI_MAX, EPI_MIN, EPI_ACT, EPI_NEG,
                     EPI_SQUARE, EPI_ABS };
enum EpiOperand : int { EPO_NONE = 0, EPO_SCALAR, EPO_SCALAR_PTR, EPO_COL, EPO_ROW, EPO_FULL };
struct EpiOp {
  int code = EPI_ADD, kind = EPO_NONE, act = ACT_NONE;
  double s = 0;              // EPO_SCALAR value
  const void* p = nullptr;   // device operand (same dtype as the output)
};
constexpr int kMaxEpi = 6;
struct EpiProg {
  int n = 0;
  EpiOp op[kMaxEpi];
};

// Output column segments (horizontally fused sibling convs): columns
// [begin[s], begin[s+1]) of the product go to their own tensor ptr[s] with
// row stride ldc[s] (column begin[s] lands at ptr[s][0]); n == 0: one output C.
constexpr int kMaxOutSegs = 4;
struct OutSegs {
  int n = 0;
  int64_t begin[kMaxOutSegs + 1];
  void* ptr[kMaxOutSegs];
  int64_t ldc[kMaxOutSegs];
  int act[kMaxOutSegs];  // per-segment activation (used in place of GemmArgs::act)
};

// C[b] = op(A[b]) @ op(B[b]) (+ bias[N]) (relu); row-major, leading dims in elements.
struct GemmArgs {
  int64_t M, N, K;
  const void* A; int64_t lda; int64_t strideA;
  const void* B; int64_t ldb; int64_t strideB;
  void* C; int64_t ldc; int64_t strideC;
  bool ta, tb;
  const void* bias;  // nullable, length N
  int act;           // epilogue activation: an Act code
  int64_t batch;
  void* workspace = nullptr;  // split-K partials (gemm_workspace_bytes)
  EpiProg epi;                // absorbed elementwise chain (epi.n == 0: none)
  OutSegs seg;                // split output (seg.n == 0: C / ldc)
};
// bytes of scratch the launch needs (0 = none); allocate before the launch
size_t gemm_workspace_bytes(DType dt, const GemmArgs& g);
void gemm(DType dt, const GemmArgs& g, hipStream_t s);
// Compute mode of float32 MatMul / Conv2D: 0 exact f32 (default), 1 bf16
// operands, 2 bf16x3 (hi/lo split, ~16-bit operands); f32 accumulate in all.
// Initial value from TFA_PRECISION (f32 | bf16 | bf16x3).
void set_f32_precision(int mode);
// Force one tile of the f32 core (-1 = heuristic + autotuner); for tests/tuning.
void set_gemm_tile(int cfg);
int gemm_tile_count();
// the autotuner's picks ({20-field shape key, tile}) and the shipped defaults
// it starts from (a default is replaced only by a >= 2 % win, confirmed twice)
std::vector<std::pair<std::vector<int64_t>, int>> gemm_tune_table();
void gemm_tune_seed(const std::vector<int64_t>& key, int cfg);
void gemm_tune_reset();
std::vector<int> gemm_tile_dims(int cfg);  // {BM, BN, core (1 round-4, 2 g2)}
int f32_precision();
// The launch one float64 GEMM takes (gemm_f64.hip): plain host code, no
// device, as reduce_route. The launch code switches on it and the tests read
// it. Whether a block is interior (unchecked 16-byte pair loads) or an edge
// block (checked loads) is decided on the device per block: a block loads A in
// pairs when its BM rows are in range and `a_pairs` holds, B likewise, and it
// runs the interleaved FAST loop when both do and `k_mult16` holds.
enum class F64Tile : int { T64x16, T64x64, T128x128, COUNT };
constexpr int64_t kGemmMaxBatchPerLaunch = 65535;  // grid.z
struct GemmF64Plan {
  F64Tile tile;
  int BM, BN;
  int64_t tiles_m, tiles_n;  // grid.x = tiles_m * tiles_n (XCD-remapped), grid.y = 1
  int64_t launches;          // slices of at most kGemmMaxBatchPerLaunch batches (grid.z)
  bool k_mult16;             // K > 0 && K % 16 == 0
  bool a_pairs, b_pairs;     // the operand is 16-byte aligned and its leading dimension even
};
const char* gemm_f64_tile_name(F64Tile t);
// a_aligned16 / b_aligned16: the operand's base address (of batch 0; a batch
// whose stride is odd moves every other matrix off the pair loads)
GemmF64Plan gemm_f64_route(int64_t M, int64_t N, int64_t K, int64_t batch, bool ta, bool tb, int64_t lda,
                           int64_t ldb, bool a_aligned16, bool b_aligned16);
// The integer GEMM: 16x16 output tiles, row-major over grid.x (column tile
// fastest), batches in grid.z slices as above.
struct GemmIntPlan {
  int64_t tiles_m, tiles_n;  // grid.x = tiles_m * tiles_n < 2^31
  int64_t launches;
};
GemmIntPlan gemm_int_route(int64_t M, int64_t N, int64_t K, int64_t batch);

// ------------------------------------------------------------ conv / pool (NHWC)
struct ConvArgs {
  int64_t N, H, W, C;       // input
  int64_t KH, KW, OC;       // filter [KH, KW, C, OC]
  int64_t OH, OW;
  int64_t sh, sw, dh, dw;
  int64_t pad_t, pad_l;
  const void* x; const void* w; void* y;
  const void* bias; int act;
  void* workspace = nullptr;
  int64_t ldc = 0;  // output pixel stride in elements (0 = OC; > OC writes a channel slice)
  EpiProg epi;      // absorbed elementwise chain over the [N*OH*OW, OC] output
  OutSegs seg;      // sibling convs fused along OC: per-sibling outputs (seg.n == 0: y / ldc)
  // Winograd filter (conv_wino_filter layout) when the planner made one:
  // 3x3 / 1x7 / 7x1 stride-1 convs then run conv_wino.hip unless TFA_CONV_ALGO=direct
  const void* wino = nullptr;
  // planner-fused 2x2 / stride 2 VALID MaxPool after the conv (and its bias /
  // activation): y is the pooled [N, OH/2, OW/2] output (ldc as above). Only
  // where conv2d_pool2_direct says so (the F(2x2,3x3) epilogue pools its own
  // 2x2 output tiles); run_conv2d falls back to conv + pool otherwise.
  bool pool2 = false;
};
size_t conv2d_workspace_bytes(DType dt, const ConvArgs& a);
void conv2d_nhwc(DType dt, const ConvArgs& a, hipStream_t s);
bool conv2d_pool2_direct(const ConvArgs& a);
// the kernel family the calling thread's last conv2d_nhwc ran ("wino_f23",
// "implicit_gemm", "gemm_1x1", "direct", ...): step-timing labels
const char* last_conv_algo();
void set_last_conv_algo(const char* label);  // a static string
const char* last_f32_tile();  // " g2 256x64" etc.: the tile of the calling thread's last f32 GEMM / conv ("" if none)
struct PoolArgs {
  int64_t N, H, W, C, OH, OW, KH, KW, sh, sw, pad_t, pad_l;
  bool is_max;
  const void* x; void* y;
  // fused epilogue (planner: Pool -> BiasAdd -> Relu/Relu6) and output pixel
  // stride (> C: the pool writes its channel slice of a concat output)
  const void* bias = nullptr;  // [C] f32 or null
  int act = 0;                 // Act code (none / relu / relu6)
  int64_t ldc = 0;             // 0 = C
};
void pool2d_nhwc(DType dt, const PoolArgs& a, hipStream_t s);
// The kernel one pool2d_nhwc() call takes (host only, as reduce_route). From
// the most to the least specialised: the unrolled 3x3 kernel (float4 channels,
// 32-bit indices) on the XCD-remapped or the plain grid, then the generic
// window loop with float4 (V4) or scalar (V1) channels and 32- or 64-bit
// index math.
enum class PoolRoute : int {
  P3X3_V4_XCD, P3X3_V4, GENERIC_V4_U32, GENERIC_V4_I64, GENERIC_V1_U32, GENERIC_V1_I64, COUNT
};
struct PoolPlan {
  PoolRoute route;
  int V;           // channels per item
  int64_t items;   // N * OH * OW * C / V
  int64_t blocks;  // grid.x
};
const char* pool_route_name(PoolRoute r);
// Only N, H, W, C, OH, OW, KH, KW and ldc of `a` are read. The result honours
// TFA_POOL_GENERIC=1 / TFA_POOL_XCD=0 and set_pool_route().
PoolPlan pool_route(const PoolArgs& a, bool x_aligned16, bool y_aligned16);
// Force a route process-wide (-1: automatic), for tests: the 64-bit index
// kernels and the plain-grid 3x3 kernel are otherwise reached only from 2^31
// elements / 2^30 blocks upward. Only a less specialised route than the
// automatic one can be forced (3x3 -> generic, xcd -> plain grid, u32 -> i64,
// v4 -> v1); pool_route() raises where the forced route asks for more than the
// shape allows.
void set_pool_route(int route);
// VALID 3x3 max pool (any stride) feeding a 1x1 / stride-1 conv (+ bias + act) in one kernel
// (conv_smallc.hip): Inception-v3 MaxPool_3a -> Conv2d_3b. The pooled tensor
// never reaches HBM. x: the pool's NHWC input; w: [C][OC]; y: [N*PH*PW][ldc].
struct PoolConvArgs {
  int64_t N, H, W, C, PH, PW, pkh, pkw, psh, psw, OC, ldc;
  const void* x; const void* w; const void* bias; void* y;
  int act = 0;
};
bool pool_conv1x1_eligible(int64_t N, int64_t H, int64_t W, int64_t C, int64_t PH, int64_t PW, int64_t OC,
                           int64_t ldc, int act);
void pool_conv1x1(const PoolConvArgs& a, hipStream_t s);
// Winograd paths (conv_wino.hip): the planner's shape test (0 none, 1
// F(2x2,3x3), 2 F(2,7) along W (1x7), 3 F(2,7) along H (7x1)), padded filter
// width, runtime switch (TFA_CONV_ALGO=direct turns it off) and forced
// kernel variant (-1 auto; >= 0 also runs OC <= 32; 3 one item per block)
int conv_wino_kind(int64_t KH, int64_t KW, int64_t sh, int64_t sw, int64_t dh, int64_t dw, int64_t C, int64_t OC);
int64_t conv_wino_ocp(int64_t OC);
int64_t conv_wino_filter_elems(int kind, int64_t C, int64_t OC);
// host: HWIO f32 filter -> the transformed filter (fp64 transform, rounded once)
void conv_wino_filter(int kind, const float* w, int64_t C, int64_t OC, float* u);
void set_conv_wino(int on);
bool conv_wino_enabled();
void set_wino_tile(int v);
void set_wino_bn(int bn);  // F(2x2,3x3) oc block: 0 auto, 32 or 64
void set_wino_5x5(int on);  // F(4,5) for 5x5 convs (opt-in; plans made after the call)
// image resize, NHWC. mode: 0 legacy (src = dst*scale), 1 align_corners, 2 half_pixel_centers
struct ResizeArgs {
  int64_t N, H, W, C, OH, OW;
  float sh, sw;  // in/out scale per axis
  int mode;
  const void* x; void* y;
};
void resize_bilinear(DType dt, const ResizeArgs& a, hipStream_t s);  // output f32
void resize_nearest(int64_t elem_size, const ResizeArgs& a, hipStream_t s);
// batched ragged image pre-stage: n uint8 HWC images of their own sizes (byte
// offsets offs[n], (H, W) pairs hw[2n]) -> f32 [n, h, w, C]: bilinear resize
// to OH x OW (mode 0 default, 1 align_corners, 2 half_pixel_centers), crop at
// (oy, ox), then up to 4 elementwise steps (0 add, 1 sub, 2 mul, 3 div; a
// scalar or per-channel constant). rp (optional, int32 [n][4]): each row's
// own OH, OW, oy, ox instead of the shared ones.
struct RaggedPrepArgs {
  int64_t n = 0;
  int C = 3, OH = 0, OW = 0, oy = 0, ox = 0, h = 0, w = 0, mode = 0;
  int nops = 0;
  int op_kind[4] = {0, 0, 0, 0}, op_chan[4] = {0, 0, 0, 0};
  float op_val[4][4] = {};
  const uint8_t* x = nullptr;
  const int64_t* offs = nullptr;
  const int32_t* hw = nullptr;
  const int32_t* rp = nullptr;
  float* y = nullptr;
};
void ragged_image_prep(const RaggedPrepArgs& a, hipStream_t s);
// ------------------------------------------------------------ wider op set (extra.hip)
// Pad / PadV2 (mode 0, constant = cbits reinterpreted as the element) and
// MirrorPad (mode 1 REFLECT, 2 SYMMETRIC); in_strides in elements
struct PadArgs {
  int rank = 0, mode = 0;
  int64_t out_dims[kMaxRank], in_dims[kMaxRank], in_strides[kMaxRank], before[kMaxRank];
};
void pad_nd(int64_t elem_size, const PadArgs& a, const void* x, void* y, uint64_t cbits, hipStream_t s);
// cumulative sum / product along the middle dim of [outer, n, inner]
void scan(bool prod, DType dt, const void* x, void* y, int64_t outer, int64_t n, int64_t inner, bool exclusive,
          bool reverse, hipStream_t s);
void leaky_relu(DType dt, const void* x, void* y, int64_t n, double alpha, hipStream_t s);
struct DepthwiseArgs {
  int64_t N, H, W, C, M, KH, KW, OH, OW, sh, sw, dh, dw, pad_t, pad_l;
  const void* x; const void* w; void* y;
};
void depthwise_conv2d_nhwc(const DepthwiseArgs& a, hipStream_t s);  // f32
void lrn(DType dt, const void* x, void* y, int64_t n, int64_t C, int radius, double bias, double alpha, double beta,
         hipStream_t s);
struct GatherNdArgs {
  int K = 0;
  int64_t dims[kMaxRank], strides[kMaxRank];  // strides in units of `inner` slices
};
void gather_nd(int64_t elem_size, DType idt, const void* params, const void* idx, void* out, int64_t nidx,
               int64_t inner, const GatherNdArgs& a, hipStream_t s);
struct WhereArgs {
  int rank = 0;
  int64_t dims[kMaxRank];
};
// pos = inclusive prefix count of mask (int64); where_coords writes [count, rank]
void mask_prefix(const uint8_t* mask, int64_t* pos, int64_t n, hipStream_t s);
void where_coords(const uint8_t* mask, const int64_t* pos, int64_t* out, int64_t n, const WhereArgs& a,
                  hipStream_t s);

// y = x * scale[c] + shift[c] (+relu), channel = last dim
void channel_affine(DType dt, const void* x, const void* scale, const void* shift, void* y,
                    int64_t n, int64_t C, int act, hipStream_t s);

}  // namespace k
}  // namespace tfa
