// Track layouts on gfx950 (include/waymotrack.h, "Track layouts"; DESIGN.md section 29 has the two definitions): the two steps
// that lie between the tracker, the post-passes and the metrics, so that the rows of a result never leave HBM.
//
//   wt_tracks_layout_*   R tracker outputs, each in buffers of its own, -> the shared layout of the post-passes (tracks_host.h):
//                        columns concatenated, CSR offsets per frame slot, and per row its trajectory numbered densely per
//                        (result, stream) by first appearance in row order.  Five launches:
//     1. sets:   the device row counts -> set_row_offsets; a negative count (the tracker's status), a count above its capacity
//                or rows beyond the outputs make every result empty and set the status.
//     2. rows:   bit-copies of the columns, the checks per row (slots ascend and lie in the packed set, categories in 1..C) and
//                frame_row_offsets by a lower-bound search per slot.
//     3. local:  one workgroup per (result, stream).  Every row puts its index into an open-addressing table keyed by its object
//                id (atomicCAS claims a slot, atomicMin keeps the earliest row of the id); a row is "first" when it holds its id's
//                minimum; an exclusive scan of the first-flags in row order is the rank by first appearance, which the first row
//                leaves in the table for the other rows of its id.  The table is in LDS up to kLdsRows rows, in the workspace above.
//     4. traj:   traj_offsets = running sum of the R x S counts, their total and their maximum.
//     5. ids:    per trajectory the object id of its first row.
//   wt_tracks_to_eval_*  K results in that layout -> the order wt_mot_*_dev take: first the rows on known ground-truth slots with
//                        a category in 1..C, by ground-truth slot and input order inside, then the others in input order.  One
//                        workgroup per result: scan of the known flags, per ground-truth slot its count, scan, scatter.
// Integers and bit-copies only: no answer depends on the order in which the atomics land.
#include "eval_device.h"
#include "tracks_layout_host.h"

using namespace wtdev;

namespace {

constexpr int kBlock = 256;                   // threads of a workgroup = rows it scans per step
constexpr int kWaves = kBlock / kWave;
constexpr int kLdsRows = 2048;                // rows of one (result, stream) up to which its table stays in LDS
constexpr int kLdsSlots = 2 * kLdsRows;       // slots of that table; a table in the workspace has 2 x the stream's rows
constexpr int kErrInvalid = 1;                // WT_ERR_INVALID
constexpr int kTable = 7;                     // entries per result of in_tables

// Exclusive prefix of v over the workgroup in thread order; *total = the sum.  Every thread calls it; scratch: kWaves entries of LDS.
__device__ __forceinline__ long long block_excl_scan(long long v, long long* scratch, long long* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long incl = v;
    for (int o = 1; o < kWave; o <<= 1) {
        const long long u = __shfl_up(incl, o, kWave);
        if (lane >= o) incl += u;
    }
    __syncthreads();                          // the sums of the call before this one have been read
    if (lane == kWave - 1) scratch[wave] = incl;
    __syncthreads();
    long long before = 0, all = 0;
    for (int k = 0; k < kWaves; ++k) {
        const long long t = scratch[k];
        if (k < wave) before += t;
        all += t;
    }
    *total = all;
    return before + incl - v;
}

// first index of a[0, n) with a[index] >= key; on unsorted data still an index in [0, n], and never smaller for a larger key
__device__ __forceinline__ long long lower_bound(const int64_t* __restrict__ a, long long n, long long key) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

template <class T>
__device__ __forceinline__ const T* table_ptr(const int64_t* __restrict__ tables, int r, int column) {
    return reinterpret_cast<const T*>((uintptr_t)tables[(size_t)r * kTable + column]);
}

struct Workspace {                            // device pointers carved from one block
    int64_t* rows;                            // [R] the row count of each result, 0 everywhere when the call is refused
    int64_t* stream_row0;                     // [R * S] the first row of the stream inside its result
    int32_t *slot, *rank;                     // [2 * out_cap] the tables of the (result, stream) above kLdsRows, at 2 x its first output row
    int32_t* first_row;                       // [out_cap] at (first output row of the stream) + t: the first row of trajectory t inside its result
    size_t bytes;
};

Workspace carve(void* base, size_t r_sets, size_t n_streams, size_t out_cap) {
    wt::Carver cv(base);
    Workspace w;
    w.rows = cv.take<int64_t>(r_sets + 1);
    w.stream_row0 = cv.take<int64_t>(r_sets * n_streams + 1);
    w.slot = cv.take<int32_t>(2 * out_cap + 1);
    w.rank = cv.take<int32_t>(2 * out_cap + 1);
    w.first_row = cv.take<int32_t>(out_cap + 1);
    w.bytes = cv.off;
    return w;
}

struct Columns {
    double *x, *y, *w, *h, *score;
    int32_t *category, *local;
};

// ---- 1. sets ----
__global__ __launch_bounds__(kBlock) void layout_sets_kernel(const int64_t* __restrict__ tables, int r_sets, long long out_cap, long long n_frames, int n_streams,
                                                             const int64_t* __restrict__ sfo, int64_t* __restrict__ set_row_offsets, Workspace ws,
                                                             int64_t* __restrict__ totals, int* __restrict__ status) {
    __shared__ long long scratch[kWaves];
    __shared__ int bad;
    const int tid = threadIdx.x;
    if (tid == 0) bad = 0;
    __syncthreads();
    long long mine = 0;
    for (int r = tid; r < r_sets; r += kBlock) {
        const long long n = *table_ptr<int64_t>(tables, r, 5), cap = tables[(size_t)r * kTable + 6];
        if (n < 0) atomicMax(&bad, (int)(-n < 0x3fffffffll ? -n : 0x3fffffffll));           // the tracker's status
        else if (n > cap || n >= wt::kLayoutMaxRows) atomicMax(&bad, kErrCapacity);
        else mine += n;
    }
    for (int s = tid; s <= n_streams; s += kBlock) {
        const long long v = sfo[s];
        if ((s == 0 && v != 0) || (s == n_streams && v != n_frames) || (s > 0 && v < sfo[s - 1])) atomicMax(&bad, kErrInvalid);
    }
    long long all;
    block_excl_scan(mine, scratch, &all);
    if (all > out_cap && tid == 0) atomicMax(&bad, kErrCapacity);
    __syncthreads();
    const int err = bad;
    long long running = 0;
    for (int b = 0; b < r_sets; b += kBlock) {
        const int r = b + tid;
        const long long n = (r < r_sets && !err) ? *table_ptr<int64_t>(tables, r, 5) : 0;
        long long total;
        const long long before = block_excl_scan(n, scratch, &total);
        if (r < r_sets) { set_row_offsets[r] = running + before; ws.rows[r] = n; }
        running += total;
    }
    if (tid == 0) {
        set_row_offsets[r_sets] = running;
        totals[0] = running;
        if (err) atomicMax(status, err);
    }
}

// ---- 2. rows ----
__global__ __launch_bounds__(kBlock) void layout_rows_kernel(const int64_t* __restrict__ tables, long long n_frames, int n_classes,
                                                             const int64_t* __restrict__ set_row_offsets, Workspace ws, Columns O,
                                                             int64_t* __restrict__ frame_row_offsets, int* __restrict__ status) {
    const int r = blockIdx.y;
    const long long n = ws.rows[r], base = set_row_offsets[r];
    const int64_t* frame = table_ptr<int64_t>(tables, r, 0);
    const int32_t* cat = table_ptr<int32_t>(tables, r, 1);
    const double* bbox = table_ptr<double>(tables, r, 2);
    const double* score = table_ptr<double>(tables, r, 3);
    const long long stride = (long long)gridDim.x * kBlock, first = (long long)blockIdx.x * kBlock + threadIdx.x;
    int err = 0;
    for (long long i = first; i < n; i += stride) {
        const long long f = frame[i];
        const int c = cat[i];
        if (f < 0 || f >= n_frames || (i > 0 && frame[i - 1] > f) || c < 1 || c > n_classes) err = kErrInvalid;
        const long long o = base + i;
        O.x[o] = bbox[4 * i + 0]; O.y[o] = bbox[4 * i + 1]; O.w[o] = bbox[4 * i + 2]; O.h[o] = bbox[4 * i + 3];
        O.score[o] = score[i];
        O.category[o] = c;
    }
    int64_t* fro = frame_row_offsets + (size_t)r * (size_t)(n_frames + 1);
    for (long long f = first; f <= n_frames; f += stride) fro[f] = lower_bound(frame, n, f);
    if (err) atomicMax(status, err);
}

// ---- 3. local ----
// the slot of `key` in a table that holds it, -1 when the table does not (it was not built from these rows)
__device__ __forceinline__ int find_slot(const int* slot, unsigned cap, const int64_t* __restrict__ id, long long ns, long long key) {
    unsigned h = wt::layout_probe(key, cap);
    for (unsigned tries = 0; tries < cap; ++tries) {
        const int v = slot[h];
        if (v < 0 || v >= ns) return -1;
        if (id[v] == key) return (int)h;
        h = h + 1 == cap ? 0 : h + 1;
    }
    return -1;
}

// The rows [0, ns) of one (result, stream), ids `id`, locals to `local`; slot / rank: cap entries each.  Returns the trajectories.
__device__ __forceinline__ long long number_by_first_appearance(int* slot, int* rank, unsigned cap, const int64_t* __restrict__ id, long long ns,
                                                                 int32_t* __restrict__ local, int32_t* __restrict__ first_row, long long row0,
                                                                 long long* scratch, int* err) {
    const int tid = threadIdx.x;
    for (unsigned h = tid; h < cap; h += kBlock) slot[h] = -1;
    __syncthreads();
    for (long long i = tid; i < ns; i += kBlock) {
        const long long key = id[i];
        unsigned h = wt::layout_probe(key, cap), tries = 0;
        for (; tries < cap; ++tries) {
            const int old = atomicCAS(&slot[h], -1, (int)i);
            if (old == -1) break;                                          // the slot is this id's from now on
            if (old >= 0 && old < ns && id[old] == key) { atomicMin(&slot[h], (int)i); break; }
            h = h + 1 == cap ? 0 : h + 1;
        }
        if (tries == cap) *err = kErrCapacity;
    }
    __syncthreads();
    long long running = 0;
    for (long long b = 0; b < ns; b += kBlock) {
        const long long i = b + tid;
        int h = -1;
        bool first = false;
        if (i < ns) {
            h = find_slot(slot, cap, id, ns, id[i]);
            if (h < 0) *err = kErrCapacity; else first = slot[h] == (int)i;
        }
        long long total;
        const long long before = block_excl_scan(first ? 1 : 0, scratch, &total);
        if (first) {
            const int t = (int)(running + before);
            rank[h] = t;
            local[i] = t;
            first_row[t] = (int)(row0 + i);
        }
        running += total;
    }
    __syncthreads();
    for (long long i = tid; i < ns; i += kBlock) {
        const int h = find_slot(slot, cap, id, ns, id[i]);
        if (h >= 0 && slot[h] != (int)i) local[i] = rank[h];
    }
    return running;
}

__global__ __launch_bounds__(kBlock) void layout_local_kernel(const int64_t* __restrict__ tables, int n_streams, const int64_t* __restrict__ sfo,
                                                              const int64_t* __restrict__ set_row_offsets, Workspace ws, int32_t* __restrict__ local,
                                                              int32_t* __restrict__ n_traj, int* __restrict__ status) {
    __shared__ int lds_slot[kLdsSlots];
    __shared__ int lds_rank[kLdsSlots];
    __shared__ long long scratch[kWaves];
    const size_t p = blockIdx.x;
    const int r = (int)(p / (size_t)n_streams), s = (int)(p % (size_t)n_streams);
    const long long n = ws.rows[r], base = set_row_offsets[r];
    const int64_t* frame = table_ptr<int64_t>(tables, r, 0);
    const int64_t* oid = table_ptr<int64_t>(tables, r, 4);
    const long long f0 = sfo[s], f1 = sfo[s + 1];
    const long long rs0 = lower_bound(frame, n, f0), rs1 = f1 > f0 ? lower_bound(frame, n, f1) : rs0;
    const long long ns = rs1 - rs0;                                        // the same in every thread
    if (threadIdx.x == 0) ws.stream_row0[p] = rs0;
    if (ns <= 0) {
        if (threadIdx.x == 0) n_traj[p] = 0;
        return;
    }
    int err = 0;
    long long T;
    if (ns <= kLdsRows)
        T = number_by_first_appearance(lds_slot, lds_rank, kLdsSlots, oid + rs0, ns, local + base + rs0, ws.first_row + base + rs0, rs0, scratch, &err);
    else
        T = number_by_first_appearance(ws.slot + 2 * (base + rs0), ws.rank + 2 * (base + rs0), (unsigned)(2 * ns), oid + rs0, ns, local + base + rs0,
                                       ws.first_row + base + rs0, rs0, scratch, &err);
    if (threadIdx.x == 0) n_traj[p] = (int)T;
    if (err) atomicMax(status, err);
}

// ---- 4. traj ----
__global__ __launch_bounds__(kBlock) void layout_traj_kernel(long long P, const int32_t* __restrict__ n_traj, int64_t* __restrict__ traj_offsets,
                                                             int64_t* __restrict__ totals) {
    __shared__ long long scratch[kWaves];
    __shared__ int most;
    const int tid = threadIdx.x;
    if (tid == 0) most = 0;
    __syncthreads();
    long long running = 0;
    int mine = 0;
    for (long long b = 0; b < P; b += kBlock) {
        const long long i = b + tid;
        const int v = i < P ? n_traj[i] : 0;
        if (v > mine) mine = v;
        long long total;
        const long long before = block_excl_scan(v, scratch, &total);
        if (i < P) traj_offsets[i] = running + before;
        running += total;
    }
    if (mine) atomicMax(&most, mine);
    __syncthreads();
    if (tid == 0) { traj_offsets[P] = running; totals[1] = running; totals[2] = most; }
}

// ---- 5. ids ----
__global__ __launch_bounds__(kBlock) void layout_ids_kernel(const int64_t* __restrict__ tables, int n_streams, const int64_t* __restrict__ set_row_offsets,
                                                            Workspace ws, const int32_t* __restrict__ n_traj, const int64_t* __restrict__ traj_offsets,
                                                            long long out_cap, int64_t* __restrict__ traj_object_id) {
    const size_t p = blockIdx.x;
    const int r = (int)(p / (size_t)n_streams);
    const long long n = ws.rows[r], at = set_row_offsets[r] + ws.stream_row0[p], t0 = traj_offsets[p];
    const int64_t* oid = table_ptr<int64_t>(tables, r, 4);
    const int T = n_traj[p];
    for (int t = threadIdx.x; t < T; t += kBlock) {
        const long long row = ws.first_row[at + t];
        if (row >= 0 && row < n && t0 + t >= 0 && t0 + t < out_cap) traj_object_id[t0 + t] = oid[row];
    }
}

int launch_layout(int64_t n_frames, int32_t n_streams, const int64_t* sfo, int32_t r_sets, const int64_t* tables, int32_t n_classes, int64_t out_cap,
                  const Columns& O, int64_t* set_row_offsets, int64_t* frame_row_offsets, int32_t* n_traj, int64_t* traj_offsets, int64_t* totals,
                  int64_t* traj_object_id, int32_t* status_dev, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    const char* entry = "wt_tracks_layout_dev";
    if (n_frames < 0 || n_streams < 0 || r_sets < 1 || n_classes < 1 || out_cap < 0 || !sfo || !tables || !O.x || !O.y || !O.w || !O.h || !O.score ||
        !O.category || !O.local || !set_row_offsets || !frame_row_offsets || !n_traj || !traj_offsets || !totals || !traj_object_id || !status_dev) {
        wt::set_error("%s: bad argument", entry);
        return WT_ERR_INVALID;
    }
    if (!wt::grid_fits((uint64_t)r_sets, (uint64_t)(n_streams > 0 ? n_streams : 1)) || r_sets > 65535) {
        wt::set_error("%s: %d results x %d streams in one call", entry, (int)r_sets, (int)n_streams);
        return WT_ERR_CAPACITY;
    }
    WT_TRY(wt::ensure_device());
    const Workspace ws = carve(wt::align_ptr(workspace), (size_t)r_sets, (size_t)n_streams, (size_t)out_cap);
    WT_TRY(wt::check_workspace_fits(entry, workspace, workspace_bytes, ws.bytes, WT_ERR_CAPACITY));
    WT_HIP(hipMemsetAsync(status_dev, 0, sizeof(int32_t), stream));
    const size_t P = (size_t)r_sets * (size_t)n_streams;
    hipLaunchKernelGGL(layout_sets_kernel, dim3(1), dim3(kBlock), 0, stream, tables, (int)r_sets, (long long)out_cap, (long long)n_frames, (int)n_streams, sfo,
                       set_row_offsets, ws, totals, (int*)status_dev);
    const long long widest = out_cap > n_frames + 1 ? out_cap : n_frames + 1;
    const unsigned gx = (unsigned)((widest + kBlock - 1) / kBlock < 256 ? (widest + kBlock - 1) / kBlock : 256);
    hipLaunchKernelGGL(layout_rows_kernel, dim3(gx, (unsigned)r_sets), dim3(kBlock), 0, stream, tables, (long long)n_frames, (int)n_classes, set_row_offsets, ws, O,
                       frame_row_offsets, (int*)status_dev);
    if (P)
        hipLaunchKernelGGL(layout_local_kernel, dim3((unsigned)P), dim3(kBlock), 0, stream, tables, (int)n_streams, sfo, set_row_offsets, ws, O.local, n_traj,
                           (int*)status_dev);
    hipLaunchKernelGGL(layout_traj_kernel, dim3(1), dim3(kBlock), 0, stream, (long long)P, n_traj, traj_offsets, totals);
    if (P)
        hipLaunchKernelGGL(layout_ids_kernel, dim3((unsigned)P), dim3(kBlock), 0, stream, tables, (int)n_streams, set_row_offsets, ws, n_traj, traj_offsets,
                           (long long)out_cap, traj_object_id);
    WT_HIP(hipGetLastError());
    return WT_OK;
}

// =====================================================================================================================
// wt_tracks_to_eval_*
struct EvalIn {
    long long n_frames, n_rows, n_gt_frames, box_stride;
    int k_sets, n_classes;
    const int64_t *set_row_offsets, *frame_row_offsets, *slot_map;
    const double *x, *y, *w, *h;
    const int32_t *category, *local;
};

struct EvalOut {
    double *x, *y, *w, *h;
    int32_t *category, *h_id;
    int64_t *set_row_offsets, *frame_hyp_offsets, *order;
    unsigned long long* max_frame_boxes;
};

__device__ __forceinline__ long long clamp_row(long long v, long long n) { return v < 0 ? 0 : (v > n ? n : v); }

// The frame slot of row i of a result (fro: its n_frames + 1 offsets), -1 when no slot holds it; *g = the ground-truth slot of a
// row that takes part (known slot, category in 1..C), -1 otherwise.
__device__ __forceinline__ long long slot_of_row(const EvalIn& I, const int64_t* __restrict__ fro, long long i, int c, long long* g, int* err) {
    *g = -1;
    long long lo = 0, hi = I.n_frames + 1;                                // first offset above i
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (fro[mid] <= i) lo = mid + 1; else hi = mid;
    }
    const long long f = lo - 1;
    if (f < 0 || f >= I.n_frames) return -1;
    const long long m = I.slot_map[f];
    if (m < -1 || m >= I.n_gt_frames) { *err = kErrInvalid; return f; }
    if (m >= 0 && c >= 1 && c <= I.n_classes) *g = m;
    return f;
}

__global__ __launch_bounds__(kBlock) void to_eval_kernel(EvalIn I, EvalOut O, int32_t* __restrict__ known_before, int* __restrict__ status) {
    __shared__ long long scratch[kWaves];
    __shared__ int most;
    const int k = blockIdx.x, tid = threadIdx.x;
    const long long lo = I.set_row_offsets[k], hi = I.set_row_offsets[k + 1], n = hi - lo, G = I.n_gt_frames;
    const int64_t* fro = I.frame_row_offsets + (size_t)k * (size_t)(I.n_frames + 1);
    int64_t* fho = O.frame_hyp_offsets + (size_t)k * (size_t)(G + 1);
    if (I.set_row_offsets[0] != 0 || lo < 0 || n < 0 || hi > I.n_rows || n >= wt::kLayoutMaxRows) {                 // the same in every thread
        for (long long g = tid; g <= G; g += kBlock) fho[g] = 0;
        if (tid == 0) { O.set_row_offsets[k] = 0; if (k == I.k_sets - 1) O.set_row_offsets[I.k_sets] = 0; atomicMax(status, kErrInvalid); }
        return;
    }
    if (tid == 0) { most = 0; O.set_row_offsets[k] = lo; if (k == I.k_sets - 1) O.set_row_offsets[I.k_sets] = hi; }
    int err = 0;
    int32_t* A = known_before + lo + k;                                   // [n + 1] the rows before row i that take part
    long long running = 0;
    for (long long b = 0; b < n; b += kBlock) {
        const long long i = b + tid;
        long long g = -1;
        if (i < n) {
            slot_of_row(I, fro, i, I.category[lo + i], &g, &err);
            if (I.local[lo + i] < 0) err = kErrInvalid;
        }
        long long total;
        const long long before = block_excl_scan(g >= 0 ? 1 : 0, scratch, &total);
        if (i < n) A[i] = (int)(running + before);
        running += total;
    }
    const long long n_on = running;
    if (tid == 0) A[n] = (int)n_on;
    for (long long g = tid; g <= G; g += kBlock) fho[g] = 0;
    __syncthreads();
    for (long long f = tid; f < I.n_frames; f += kBlock) {                // the map is injective: one writer per ground-truth slot
        const long long g = I.slot_map[f];
        if (g < 0 || g >= G) continue;
        long long count = (long long)A[clamp_row(fro[f + 1], n)] - (long long)A[clamp_row(fro[f], n)];
        if (count < 0) { err = kErrInvalid; count = 0; }
        fho[g] = count;
    }
    __syncthreads();
    running = 0;
    for (long long b = 0; b < G; b += kBlock) {
        const long long g = b + tid;
        const long long v = g < G ? fho[g] : 0;
        long long total;
        const long long before = block_excl_scan(v, scratch, &total);
        if (g < G) fho[g] = running + before;
        running += total;
    }
    if (tid == 0) fho[G] = running;
    if (running != n_on) err = kErrInvalid;                               // two frame slots named one ground-truth slot, or the offsets descend
    __syncthreads();
    int mine = 0;
    for (long long i = tid; i < n; i += kBlock) {
        const int c = I.category[lo + i];
        long long g;
        const long long f = slot_of_row(I, fro, i, c, &g, &err);
        long long pos;
        if (g >= 0) {
            const long long f_row0 = clamp_row(fro[f], n);
            pos = fho[g] + ((long long)A[i] - (long long)A[f_row0]);
            if (pos < 0 || pos >= n_on) { err = kErrInvalid; continue; }
            int same = 1;                                                 // rows of this class in the slot up to this one
            for (long long j = f_row0; j < i; ++j) same += I.category[lo + j] == c;
            if (same > mine) mine = same;
        } else {
            pos = n_on + (i - (long long)A[i]);
            if (pos < n_on || pos >= n) { err = kErrInvalid; continue; }
        }
        const long long src = (lo + i) * I.box_stride, o = lo + pos;
        O.x[o] = I.x[src]; O.y[o] = I.y[src]; O.w[o] = I.w[src]; O.h[o] = I.h[src];
        O.category[o] = c;
        O.h_id[o] = I.local[lo + i];
        O.order[o] = i;
    }
    if (mine) atomicMax(&most, mine);
    if (err) atomicMax(status, err);
    __syncthreads();
    if (tid == 0 && most) atomicMax(O.max_frame_boxes, (unsigned long long)most);
}

size_t to_eval_bytes(size_t k_sets, size_t n_rows) {
    wt::Carver cv(nullptr);
    cv.take<int32_t>(n_rows + k_sets + 1);
    return cv.off;
}

int launch_to_eval(const EvalIn& I, const EvalOut& O, int32_t* status_dev, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    const char* entry = "wt_tracks_to_eval_dev";
    if (I.n_frames < 0 || I.k_sets < 1 || I.n_rows < 0 || I.n_gt_frames < 0 || I.n_classes < 1 || I.box_stride < 1 || !I.set_row_offsets || !I.frame_row_offsets ||
        !I.slot_map || !I.x || !I.y || !I.w || !I.h || !I.category || !I.local || !O.x || !O.y || !O.w || !O.h || !O.category || !O.h_id || !O.set_row_offsets ||
        !O.frame_hyp_offsets || !O.order || !O.max_frame_boxes || !status_dev) {
        wt::set_error("%s: bad argument", entry);
        return WT_ERR_INVALID;
    }
    WT_TRY(wt::ensure_device());
    WT_TRY(wt::check_workspace_fits(entry, workspace, workspace_bytes, to_eval_bytes((size_t)I.k_sets, (size_t)I.n_rows), WT_ERR_CAPACITY));
    WT_HIP(hipMemsetAsync(status_dev, 0, sizeof(int32_t), stream));
    WT_HIP(hipMemsetAsync(O.max_frame_boxes, 0, sizeof(int64_t), stream));
    hipLaunchKernelGGL(to_eval_kernel, dim3((unsigned)I.k_sets), dim3(kBlock), 0, stream, I, O, reinterpret_cast<int32_t*>(wt::align_ptr(workspace)),
                       (int*)status_dev);
    WT_HIP(hipGetLastError());
    return WT_OK;
}

// wait for the launches and read the kernels' status
int finish(const wt::DevBuf& status, const char* what) {
    WT_HIP(hipDeviceSynchronize());
    int32_t st = 0;
    WT_HIP(hipMemcpy(&st, status.p, sizeof(st), hipMemcpyDeviceToHost));
    if (st) wt::set_error("%s kernel reported status %d", what, (int)st);
    return (int)st;
}

}  // namespace

extern "C" {

void wt_tracks_layout_limits(int32_t* lds_rows, int32_t* lds_slots, int32_t* scan_rows) {
    if (lds_rows) *lds_rows = kLdsRows;
    if (lds_slots) *lds_slots = kLdsSlots;
    if (scan_rows) *scan_rows = kBlock;
}

int32_t wt_tracks_layout_probe(int64_t id, int32_t capacity) {
    return capacity < 1 ? -1 : (int32_t)wt::layout_probe(id, (uint32_t)capacity);
}

size_t wt_tracks_layout_workspace(int32_t r_sets, int32_t n_streams, int64_t out_cap) {
    if (r_sets < 1 || n_streams < 0 || out_cap < 0) return 0;
    return carve(nullptr, (size_t)r_sets, (size_t)n_streams, (size_t)out_cap).bytes + 256;
}

int wt_tracks_layout_dev(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets, int32_t r_sets, const int64_t* in_tables,
                         int32_t n_classes, int64_t out_cap,
                         double* x, double* y, double* w, double* h, double* score, int32_t* category, int32_t* local,
                         int64_t* set_row_offsets, int64_t* frame_row_offsets, int32_t* n_traj, int64_t* traj_offsets, int64_t* totals,
                         int64_t* traj_object_id, int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream) {
    const Columns O = {x, y, w, h, score, category, local};
    return launch_layout(n_frames, n_streams, stream_frame_offsets, r_sets, in_tables, n_classes, out_cap, O, set_row_offsets, frame_row_offsets, n_traj,
                         traj_offsets, totals, traj_object_id, status_dev, workspace, workspace_bytes, (hipStream_t)stream);
}

int wt_tracks_layout_host(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets, int32_t r_sets, const int64_t* in_row_offsets,
                          const int64_t* in_frame, const int32_t* in_category, const double* in_bbox, const double* in_score, const int64_t* in_object_id,
                          int32_t n_classes,
                          double* x, double* y, double* w, double* h, double* score, int32_t* category, int32_t* local,
                          int64_t* set_row_offsets, int64_t* frame_row_offsets, int32_t* n_traj, int64_t* traj_offsets, int64_t* totals,
                          int64_t* traj_object_id) {
    const wt::LayoutInput in = {n_frames, n_streams, stream_frame_offsets, r_sets, in_row_offsets, in_frame, in_category, in_bbox, in_score, in_object_id, n_classes};
    int64_t max_rows = 0, n_rows = 0;
    WT_TRY(wt::check_layout_input(in, &max_rows, &n_rows));
    if (!set_row_offsets || !frame_row_offsets || !n_traj || !traj_offsets || !totals ||
        (n_rows > 0 && !(x && y && w && h && score && category && local && traj_object_id))) {
        wt::set_error("wt_tracks_layout_host: bad argument");
        return WT_ERR_INVALID;
    }
    WT_TRY(wt::ensure_device());
    const size_t N = (size_t)n_rows, R = (size_t)r_sets, nf = (size_t)(n_frames + 1), P = R * (size_t)n_streams;
    wt::DevBuf so, df, dc, db, ds, di, dn, dt, ox, oy, ow, oh, os, oc, ol, osr, ofr, ont, oto, otot, oid, status, dws;
    WT_TRY(so.upload(stream_frame_offsets, 8 * (size_t)(n_streams + 1)));
    WT_TRY(df.upload(in_frame, 8 * N)); WT_TRY(dc.upload(in_category, 4 * N)); WT_TRY(db.upload(in_bbox, 32 * N)); WT_TRY(ds.upload(in_score, 8 * N));
    WT_TRY(di.upload(in_object_id, 8 * N));
    std::vector<int64_t> counts(R), tables(R * kTable);               // every result's buffers are a part of the staged columns
    WT_TRY(dn.alloc(8 * R));
    for (size_t r = 0; r < R; ++r) {
        const size_t at = (size_t)in_row_offsets[r];
        counts[r] = in_row_offsets[r + 1] - in_row_offsets[r];
        int64_t* t = &tables[r * kTable];
        t[0] = (int64_t)(uintptr_t)(df.as<int64_t>() + at); t[1] = (int64_t)(uintptr_t)(dc.as<int32_t>() + at); t[2] = (int64_t)(uintptr_t)(db.as<double>() + 4 * at);
        t[3] = (int64_t)(uintptr_t)(ds.as<double>() + at); t[4] = (int64_t)(uintptr_t)(di.as<int64_t>() + at); t[5] = (int64_t)(uintptr_t)(dn.as<int64_t>() + r);
        t[6] = counts[r];
    }
    WT_HIP(hipMemcpy(dn.p, counts.data(), 8 * R, hipMemcpyHostToDevice));
    WT_TRY(dt.upload(tables.data(), 8 * R * kTable));
    WT_TRY(ox.alloc(8 * N)); WT_TRY(oy.alloc(8 * N)); WT_TRY(ow.alloc(8 * N)); WT_TRY(oh.alloc(8 * N)); WT_TRY(os.alloc(8 * N)); WT_TRY(oc.alloc(4 * N));
    WT_TRY(ol.alloc(4 * N)); WT_TRY(osr.alloc(8 * (R + 1))); WT_TRY(ofr.alloc(8 * R * nf)); WT_TRY(ont.alloc(4 * P)); WT_TRY(oto.alloc(8 * (P + 1)));
    WT_TRY(otot.alloc(24)); WT_TRY(oid.alloc(8 * N)); WT_TRY(status.alloc(16));
    const size_t wsb = wt_tracks_layout_workspace(r_sets, n_streams, n_rows);
    WT_TRY(dws.alloc(wsb));
    const Columns O = {ox.as<double>(), oy.as<double>(), ow.as<double>(), oh.as<double>(), os.as<double>(), oc.as<int32_t>(), ol.as<int32_t>()};
    WT_TRY(launch_layout(n_frames, n_streams, so.as<int64_t>(), r_sets, dt.as<int64_t>(), n_classes, n_rows, O, osr.as<int64_t>(), ofr.as<int64_t>(),
                         ont.as<int32_t>(), oto.as<int64_t>(), otot.as<int64_t>(), oid.as<int64_t>(), status.as<int32_t>(), dws.p, wsb, nullptr));
    WT_TRY(finish(status, "track layout"));
    if (N) {
        WT_HIP(hipMemcpy(x, ox.p, 8 * N, hipMemcpyDeviceToHost)); WT_HIP(hipMemcpy(y, oy.p, 8 * N, hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(w, ow.p, 8 * N, hipMemcpyDeviceToHost)); WT_HIP(hipMemcpy(h, oh.p, 8 * N, hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(score, os.p, 8 * N, hipMemcpyDeviceToHost)); WT_HIP(hipMemcpy(category, oc.p, 4 * N, hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(local, ol.p, 4 * N, hipMemcpyDeviceToHost));
    }
    WT_HIP(hipMemcpy(totals, otot.p, 24, hipMemcpyDeviceToHost));
    if (totals[1] > 0) WT_HIP(hipMemcpy(traj_object_id, oid.p, 8 * (size_t)totals[1], hipMemcpyDeviceToHost));
    WT_HIP(hipMemcpy(set_row_offsets, osr.p, 8 * (R + 1), hipMemcpyDeviceToHost));
    WT_HIP(hipMemcpy(frame_row_offsets, ofr.p, 8 * R * nf, hipMemcpyDeviceToHost));
    if (P) WT_HIP(hipMemcpy(n_traj, ont.p, 4 * P, hipMemcpyDeviceToHost));
    WT_HIP(hipMemcpy(traj_offsets, oto.p, 8 * (P + 1), hipMemcpyDeviceToHost));
    return WT_OK;
}

size_t wt_tracks_to_eval_workspace(int32_t k_sets, int64_t n_rows) {
    if (k_sets < 1 || n_rows < 0) return 0;
    return to_eval_bytes((size_t)k_sets, (size_t)n_rows) + 256;
}

int wt_tracks_to_eval_dev(int64_t n_frames, int32_t k_sets, int64_t n_rows, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                          const double* x, const double* y, const double* w, const double* h, int64_t box_stride,
                          const int32_t* category, const int32_t* local, const int64_t* slot_map, int64_t n_gt_frames, int32_t n_classes,
                          double* out_x, double* out_y, double* out_w, double* out_h, int32_t* out_category, int32_t* out_h_id,
                          int64_t* out_set_row_offsets, int64_t* frame_hyp_offsets, int64_t* out_order, int64_t* max_frame_boxes,
                          int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream) {
    const EvalIn I = {n_frames, n_rows, n_gt_frames, box_stride, k_sets, n_classes, set_row_offsets, frame_row_offsets, slot_map, x, y, w, h, category, local};
    const EvalOut O = {out_x, out_y, out_w, out_h, out_category, out_h_id, out_set_row_offsets, frame_hyp_offsets, out_order,
                       reinterpret_cast<unsigned long long*>(max_frame_boxes)};
    return launch_to_eval(I, O, status_dev, workspace, workspace_bytes, (hipStream_t)stream);
}

int wt_tracks_to_eval_host(int64_t n_frames, int32_t k_sets, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                           const double* x, const double* y, const double* w, const double* h, int64_t box_stride,
                           const int32_t* category, const int32_t* local, const int64_t* slot_map, int64_t n_gt_frames, int32_t n_classes,
                           double* out_x, double* out_y, double* out_w, double* out_h, int32_t* out_category, int32_t* out_h_id,
                           int64_t* out_set_row_offsets, int64_t* frame_hyp_offsets, int64_t* out_order, int64_t* max_frame_boxes) {
    const wt::ToEvalInput in = {n_frames, k_sets, set_row_offsets, frame_row_offsets, x, y, w, h, box_stride, category, local, slot_map, n_gt_frames, n_classes};
    int64_t max_slot_rows = 0, n_rows = 0;
    WT_TRY(wt::check_to_eval_input(in, &max_slot_rows, &n_rows));
    if (!out_set_row_offsets || !frame_hyp_offsets || !max_frame_boxes ||
        (n_rows > 0 && !(out_x && out_y && out_w && out_h && out_category && out_h_id && out_order))) {
        wt::set_error("wt_tracks_to_eval_host: bad argument");
        return WT_ERR_INVALID;
    }
    WT_TRY(wt::ensure_device());
    const size_t N = (size_t)n_rows, K = (size_t)k_sets, nf = (size_t)(n_frames + 1), ng = (size_t)(n_gt_frames + 1), B = 8 * N * (size_t)box_stride;
    wt::DevBuf sr, fr, dx, dy, dw, dh, dc, dl, dm, ox, oy, ow, oh, oc, oi, osr, ofh, oo, om, status, dws;
    WT_TRY(sr.upload(set_row_offsets, 8 * (K + 1))); WT_TRY(fr.upload(frame_row_offsets, 8 * K * nf));
    // with a stride the four columns are one array of rows: stage each from its own first element
    WT_TRY(dx.upload(x, B ? B - 8 * (size_t)(box_stride - 1) : 0)); WT_TRY(dy.upload(y, B ? B - 8 * (size_t)(box_stride - 1) : 0));
    WT_TRY(dw.upload(w, B ? B - 8 * (size_t)(box_stride - 1) : 0)); WT_TRY(dh.upload(h, B ? B - 8 * (size_t)(box_stride - 1) : 0));
    WT_TRY(dc.upload(category, 4 * N)); WT_TRY(dl.upload(local, 4 * N)); WT_TRY(dm.upload(slot_map, 8 * (size_t)n_frames));
    WT_TRY(ox.alloc(8 * N)); WT_TRY(oy.alloc(8 * N)); WT_TRY(ow.alloc(8 * N)); WT_TRY(oh.alloc(8 * N)); WT_TRY(oc.alloc(4 * N)); WT_TRY(oi.alloc(4 * N));
    WT_TRY(osr.alloc(8 * (K + 1))); WT_TRY(ofh.alloc(8 * K * ng)); WT_TRY(oo.alloc(8 * N)); WT_TRY(om.alloc(16)); WT_TRY(status.alloc(16));
    const size_t wsb = wt_tracks_to_eval_workspace(k_sets, n_rows);
    WT_TRY(dws.alloc(wsb));
    const EvalIn I = {n_frames, n_rows, n_gt_frames, box_stride, k_sets, n_classes, sr.as<int64_t>(), fr.as<int64_t>(), dm.as<int64_t>(), dx.as<double>(),
                      dy.as<double>(), dw.as<double>(), dh.as<double>(), dc.as<int32_t>(), dl.as<int32_t>()};
    const EvalOut O = {ox.as<double>(), oy.as<double>(), ow.as<double>(), oh.as<double>(), oc.as<int32_t>(), oi.as<int32_t>(), osr.as<int64_t>(),
                       ofh.as<int64_t>(), oo.as<int64_t>(), om.as<unsigned long long>()};
    WT_TRY(launch_to_eval(I, O, status.as<int32_t>(), dws.p, wsb, nullptr));
    WT_TRY(finish(status, "tracks to eval"));
    if (N) {
        WT_HIP(hipMemcpy(out_x, ox.p, 8 * N, hipMemcpyDeviceToHost)); WT_HIP(hipMemcpy(out_y, oy.p, 8 * N, hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(out_w, ow.p, 8 * N, hipMemcpyDeviceToHost)); WT_HIP(hipMemcpy(out_h, oh.p, 8 * N, hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(out_category, oc.p, 4 * N, hipMemcpyDeviceToHost)); WT_HIP(hipMemcpy(out_h_id, oi.p, 4 * N, hipMemcpyDeviceToHost));
        WT_HIP(hipMemcpy(out_order, oo.p, 8 * N, hipMemcpyDeviceToHost));
    }
    WT_HIP(hipMemcpy(out_set_row_offsets, osr.p, 8 * (K + 1), hipMemcpyDeviceToHost));
    WT_HIP(hipMemcpy(frame_hyp_offsets, ofh.p, 8 * K * ng, hipMemcpyDeviceToHost));
    WT_HIP(hipMemcpy(max_frame_boxes, om.p, 8, hipMemcpyDeviceToHost));
    return WT_OK;
}

}  // extern "C"
