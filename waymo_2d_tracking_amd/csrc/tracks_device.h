// Device side shared by the track post-passes (track_refine.hip, track_stitch.hip, track_smooth.hip, track_dedup.hip,
// track_split.hip, track_xclass.hip; DESIGN.md section 20, "The shared layer"): the layout all six take - R results over the frame slots of S streams, CSR offsets, a dense
// per-stream trajectory index per row, J jobs that each name a result - the rows and trajectories of one (result, stream) with
// every bound checked once, and the walk of a wavefront over them.
// Include it after eval_device.h, only from units compiled with -ffp-contract=off.
#pragma once
#include "eval_device.h"

namespace wtdev {

struct TrackLayout {                          // device pointers; a stage's Layout is this plus its own job parameters
    long long n_frames, n_rows, n_traj_total, max_traj;
    int n_streams, r_sets, n_jobs, n_classes, lds_traj;
    const int64_t *stream_frame_offsets, *set_row_offsets, *frame_row_offsets, *traj_offsets;
    const int32_t *category, *local, *job_result;
};

// The rows and trajectories of one (result r, stream s).  ok = false: the caller's numbers do not fit (status).
struct Span {
    int T;
    long long f0, f1, base, rend, rs0, t0;
    const int64_t* fro;
    bool ok;
};

__device__ __forceinline__ Span span_of(const TrackLayout& L, int r, int s) {
    Span q;
    q.ok = r >= 0 && r < L.r_sets;
    if (!q.ok) return q;
    const size_t rs = (size_t)r * L.n_streams + s;
    const long long t0 = L.traj_offsets[rs], t1 = L.traj_offsets[rs + 1];
    q.f0 = L.stream_frame_offsets[s];
    q.f1 = L.stream_frame_offsets[s + 1];
    q.base = L.set_row_offsets[r];
    q.rend = L.set_row_offsets[r + 1];
    q.fro = L.frame_row_offsets + (size_t)r * (size_t)(L.n_frames + 1);
    q.ok = t0 >= 0 && t1 >= t0 && t1 - t0 <= L.max_traj && t1 <= L.n_traj_total && q.f0 >= 0 && q.f1 >= q.f0 && q.f1 <= L.n_frames &&
           q.f1 - q.f0 < 0x3fffffffll && q.base >= 0 && q.rend >= q.base && q.rend <= L.n_rows;
    if (!q.ok) return q;
    q.T = (int)(t1 - t0);
    q.t0 = t0;
    q.rs0 = q.f1 > q.f0 ? q.base + q.fro[q.f0] : q.base;
    q.ok = q.rs0 >= q.base && q.rs0 <= q.rend;
    return q;
}

// rows [r0, r1) of slot f, or false when they leave the result's rows
__device__ __forceinline__ bool slot_rows(const Span& q, long long f, long long* r0, long long* r1) {
    *r0 = q.base + q.fro[f];
    *r1 = q.base + q.fro[f + 1];
    return *r0 >= q.rs0 && *r1 >= *r0 && *r1 <= q.rend && *r1 - q.rs0 < 0x7fffffffll;
}

// one past the stream's last row; when that leaves the result's rows, *err = kErrCapacity and the stream counts as empty
__device__ __forceinline__ long long stream_end(const Span& q, int* err) {
    if (q.f1 <= q.f0) return q.rs0;
    const long long end = q.base + q.fro[q.f1];
    if (end < q.rs0 || end > q.rend || end - q.rs0 >= 0x7fffffffll) { *err = kErrCapacity; return q.rs0; }
    return end;
}

// One wavefront walks the span's slots in order, the rows of a slot lane-parallel in chunks of 64: body(d, t, slot) for row d of
// trajectory t = local[d], slot counted from the stream's first.  Local indices are unique inside a slot, so the lanes of a chunk
// never meet in a per-trajectory table; the wavefront is synchronised after every slot.  A slot whose rows leave the result's
// ends the walk, a row whose index is outside [0, T) is skipped; either sets *err = kErrCapacity in the lanes that saw it.
template <class Body>
__device__ __forceinline__ void for_stream_rows(const Span& q, const int32_t* local, int* err, Body body) {
    const int lane = threadIdx.x & 63;
    for (long long f = q.f0; f < q.f1; ++f) {
        long long r0, r1;
        if (!slot_rows(q, f, &r0, &r1)) { *err = kErrCapacity; break; }
        for (long long b = r0; b < r1; b += kWave) {
            const long long d = b + lane;
            if (d >= r1) continue;
            const int t = local[d];
            if (t < 0 || t >= q.T) { *err = kErrCapacity; continue; }
            body(d, t, (int)(f - q.f0));
        }
        wsync();
    }
}

}  // namespace wtdev
