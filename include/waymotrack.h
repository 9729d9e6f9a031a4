/* libwaymotrack - C ABI of the MI355X-native detect -> ensemble -> SORT hot path.
 *
 * The reference (xuyuan/waymo_2d_tracking) is pure Python and has no FFI layer: its "operator API" is a
 * set of Python call signatures.  Each entry point below replaces one of those
 * call sites; the Python shims in waymo_2d_tracking_amd/ keep the reference's names and argument
 * meaning and reach this library through ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions: C linkage, plain pointers and sizes, no exceptions; every function returns an int status
 * (WT_OK == 0) and wt_last_error() gives the message of the calling thread's last failure.  All compute
 * runs in HIP kernels on the current HIP device (gfx950); there is NO CPU fallback: without a usable GPU
 * the functions return WT_ERR_NO_DEVICE.
 *   *_host entry points take host buffers (they stage through device memory internally);
 *   *_dev  entry points take device pointers plus a hipStream_t (passed as void*), never synchronise,
 *          and use only caller-provided workspace (query the size with the matching *_workspace call).
 * Paths below are relative to the reference repository root.
 */
#ifndef WAYMOTRACK_H
#define WAYMOTRACK_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define WT_OK 0
#define WT_ERR_INVALID 1    /* bad argument */
#define WT_ERR_NO_DEVICE 2  /* no HIP device / wrong architecture */
#define WT_ERR_HIP 3        /* HIP runtime error */
#define WT_ERR_CAPACITY 4   /* caller buffer or workspace too small */
#define WT_ERR_NUMERIC 5    /* iteration guard hit inside a kernel (e.g. NaN cost matrix) */

const char* wt_last_error(void);
/* ABI version of this header (bumped on any signature change). */
int wt_abi_version(void);
/* Number of visible HIP devices and name/arch of the current one ("gfx950..."). */
int wt_device_info(int* n_devices, char* arch, int arch_cap, int* n_cu);

/* =================================================================================================
 * SORT  (tracking/sort/sort.py, tracking/sort/tracker_sort.py, tracking/utils.py)
 * ================================================================================================= */

/* Process-global track-ID counter: KalmanBoxTracker.count (tracking/sort/sort.py:86,140-141). */
typedef struct wt_idctr wt_idctr;
wt_idctr* wt_idctr_create(int64_t start);
int64_t wt_idctr_get(const wt_idctr* c);
void wt_idctr_set(wt_idctr* c, int64_t value);
void wt_idctr_destroy(wt_idctr* c);

/* Sort(max_age, min_hits) - tracking/sort/sort.py:234-242.  State lives in device memory.
 * ctr may be NULL (private counter starting at 0). */
typedef struct wt_sort wt_sort;
int wt_sort_create(int max_age, int min_hits, wt_idctr* ctr, wt_sort** out);
void wt_sort_destroy(wt_sort* s);
/* Sort.update(dets, iou_threshold) - tracking/sort/sort.py:244-296.
 * dets5: (n,5) float32 rows [x1,y1,x2,y2,score] (n may be 0: "must be called once per frame even with empty
 * detections", :248).  out6: up to cap rows [x1,y1,x2,y2,id+1,confidence] float64, newest track first. */
int wt_sort_update_host(wt_sort* s, const float* dets5, int n, double iou_threshold,
                        double* out6, int cap, int* n_out);
/* Number of live tracks (len(self.trackers)) after the last update. */
int wt_sort_num_tracks(const wt_sort* s);
/* Debug/test hook: current track list in list order (ids, state x[7], covariance P[49], row-major). */
int wt_sort_state_host(wt_sort* s, int cap, int64_t* ids, double* x7, double* P49, int* n_tracks);

/* MultiClassTrackerSort(max_age, min_hits) - tracking/sort/tracker_sort.py:10-51: one Sort per class, created the first
 * time the class is seen; every known class is updated once per call, in first-seen order.
 *   dets6          : (n,6) float64 rows [x1,y1,x2,y2,confidence,class] (class = integer >= 1), cast to float32 like
 *                    np.array(..., dtype=np.float32) (:45)
 *   iou_thresholds : iou_thresholds[class-1] (:49); a class beyond n_thresholds is WT_ERR_INVALID (IndexError there)
 *   out6           : rows [x1,y1,x2,y2,id+1,confidence] of all classes, grouped by class in first-seen order;
 *   out_classes[k] / out_counts[k] : class id and row count of group k (k < *n_classes <= class_cap)
 * wt_mct_tracker returns the class's Sort (borrowed; NULL if the class has not been seen) for wt_sort_state_host. */
typedef struct wt_mct wt_mct;
int wt_mct_create(int max_age, int min_hits, wt_idctr* ctr, wt_mct** out);
void wt_mct_destroy(wt_mct* m);
int wt_mct_num_classes(const wt_mct* m);
wt_sort* wt_mct_tracker(wt_mct* m, int class_id);
int wt_mct_track_host(wt_mct* m, const double* dets6, int n, const double* iou_thresholds, int n_thresholds,
                      double* out6, int cap, int32_t* out_classes, int32_t* out_counts, int class_cap, int* n_classes);

/* associate_detections_to_trackers(detections, trackers, iou_threshold) - tracking/sort/sort.py:193-230
 * (IoU matrix :33-47,201-205 + sklearn 0.22.2 linear_assignment :206 + threshold filter :218-224).
 * dets5 (n,5) f32, trks4 (t,4) f64.  matches: (det,trk) pairs sorted by det; unmatched lists in the
 * reference's order.  Buffers: matches 2*min(n,t), unmatched_dets n, unmatched_trks t ints. */
int wt_associate_host(const float* dets5, int n, const double* trks4, int t, double iou_threshold,
                      int* matches, int* n_matches, int* unmatched_dets, int* n_unmatched_dets,
                      int* unmatched_trks, int* n_unmatched_trks);

/* linear_assignment(X) of scikit-learn 0.22.2 (call site tracking/sort/sort.py:206) on a float32 cost matrix
 * (n_rows x n_cols, row-major).  pairs: (row,col) sorted by row, 2*min(n_rows,n_cols) ints. */
int wt_linear_assignment_f32_host(const float* cost, int n_rows, int n_cols, int* pairs, int* n_pairs);

/* Batched tracking of every (segment,camera) stream of a detections file:
 * read_data_file filters (tracking/utils.py:79,86) + track_sort (tracking/utils.py:25-60) +
 * MultiClassTrackerSort.track (tracking/sort/tracker_sort.py:22-51) in the stream order of
 * tracking/track.py:43-47, including the global ID order of tracking/sort/sort.py:86.
 *
 * Detections are SoA, sorted by (stream, frame) with the input order preserved inside a frame:
 *   x,y,w,h,score float64 (JSON numbers), category int32 in 1..n_classes.
 * frame_det_offsets (n_frames+1) and stream_frame_offsets (n_streams+1) are CSR offsets; frames of a stream
 * are in ascending frame-id order; a frame whose detections are all filtered still ticks the trackers.
 * clip_w/clip_h: per-stream image size (tracking/utils.py:11-22); <= 0 disables clipping, the w/h<1 drop and
 * the confidence clip.  score_threshold / iou_threshold: n_classes entries indexed by category-1.
 * id_base: value of the global ID counter before this call (rank offset in multi-GPU runs).
 * Outputs hold at most n_dets rows, in the reference's output order:
 *   out_frame (global frame index), out_category, out_bbox4 [x1,y1,w,h], out_score, out_object_id.
 * n_births = number of track IDs consumed. */
typedef struct wt_track_params {
    int32_t max_age;
    int32_t min_hits;
    int32_t n_classes;
    int32_t reserved;
    const double* score_threshold;   /* host pointers, n_classes entries */
    const double* iou_threshold;
} wt_track_params;

int wt_track_streams_host(int64_t n_dets, const double* x, const double* y, const double* w, const double* h,
                          const double* score, const int32_t* category,
                          int64_t n_frames, const int64_t* frame_det_offsets,
                          int32_t n_streams, const int64_t* stream_frame_offsets,
                          const double* clip_w, const double* clip_h,
                          const wt_track_params* params, int64_t id_base,
                          int64_t* out_frame, int32_t* out_category, double* out_bbox4, double* out_score,
                          int64_t* out_object_id, int64_t* n_out, int64_t* n_births);

/* Device-resident form.  All array arguments are device pointers except params (host struct with host
 * threshold arrays) ; max_frame_dets = max detections in any frame (sizes the per-tracker state).
 * n_out_dev / n_births_dev: device int64 scalars.  Stream-ordered on `stream`; no host synchronisation. */
size_t wt_track_streams_workspace(int64_t n_dets, int64_t n_frames, int32_t n_streams, int64_t max_frame_dets,
                                  const wt_track_params* params);
int wt_track_streams_dev(int64_t n_dets, const double* x, const double* y, const double* w, const double* h,
                         const double* score, const int32_t* category,
                         int64_t n_frames, const int64_t* frame_det_offsets,
                         int32_t n_streams, const int64_t* stream_frame_offsets,
                         const double* clip_w, const double* clip_h, int64_t max_frame_dets,
                         const wt_track_params* params, int64_t id_base,
                         int64_t* out_frame, int32_t* out_category, double* out_bbox4, double* out_score,
                         int64_t* out_object_id, int64_t* n_out_dev, int64_t* n_births_dev,
                         void* workspace, size_t workspace_bytes, void* stream);

/* The same batched tracking with a second association over low-score detections (ByteTrack, Zhang et al., ECCV 2022).
 * Arguments as the wt_track_streams_* twins, plus low_score_threshold / low_iou_threshold: host arrays, n_classes entries
 * indexed by category-1.  params->score_threshold stays the HIGH threshold.
 *   A detection is valid when its category is in 1..n_classes, !(w < 1), !(h < 1) and !(score < low_score_threshold[c]);
 *   a valid one is high when !(score < score_threshold[c]), otherwise low.
 *   A class's tracker is created, and the class's place in the id order fixed, by its first valid detection, high or low.
 *   Per frame and class: predict; associate the high detections with all tracks (iou_threshold[c]); associate the low ones
 *   with the tracks left unmatched, in list order (low_iou_threshold[c]); both kinds of match update their track alike;
 *   births from unmatched high detections only; emit and reap as before.  A low detection without a track is dropped.
 * With low_score_threshold == score_threshold nothing is low and the rows are those of wt_track_streams_*.
 * WT_ERR_INVALID (the message names the class) when low_score_threshold[c] > score_threshold[c], when a threshold is NaN or
 * when low_iou_threshold[c] is outside [0, 1]; checked before any device call.  wt_track_streams_byte_workspace returns 0 then.
 * Batch form only: the streaming entry points below, wt_sort_* and wt_mct_* have no second association. */
int wt_track_streams_byte_host(int64_t n_dets, const double* x, const double* y, const double* w, const double* h,
                               const double* score, const int32_t* category,
                               int64_t n_frames, const int64_t* frame_det_offsets,
                               int32_t n_streams, const int64_t* stream_frame_offsets,
                               const double* clip_w, const double* clip_h,
                               const wt_track_params* params, const double* low_score_threshold,
                               const double* low_iou_threshold, int64_t id_base,
                               int64_t* out_frame, int32_t* out_category, double* out_bbox4, double* out_score,
                               int64_t* out_object_id, int64_t* n_out, int64_t* n_births);
size_t wt_track_streams_byte_workspace(int64_t n_dets, int64_t n_frames, int32_t n_streams, int64_t max_frame_dets,
                                       const wt_track_params* params, const double* low_score_threshold,
                                       const double* low_iou_threshold);
int wt_track_streams_byte_dev(int64_t n_dets, const double* x, const double* y, const double* w, const double* h,
                              const double* score, const int32_t* category,
                              int64_t n_frames, const int64_t* frame_det_offsets,
                              int32_t n_streams, const int64_t* stream_frame_offsets,
                              const double* clip_w, const double* clip_h, int64_t max_frame_dets,
                              const wt_track_params* params, const double* low_score_threshold,
                              const double* low_iou_threshold, int64_t id_base,
                              int64_t* out_frame, int32_t* out_category, double* out_bbox4, double* out_score,
                              int64_t* out_object_id, int64_t* n_out_dev, int64_t* n_births_dev,
                              void* workspace, size_t workspace_bytes, void* stream);

/* Streaming form of the same tracker (online detect -> track: tracking/utils.py:29-36 keeps ONE MultiClassTrackerSort per
 * stream alive while the frames arrive).  The trackers of n_streams streams live in a caller-owned device block `state`;
 * every wt_track_chunk_dev call feeds the next frames of each stream (same SoA / CSR layout as wt_track_streams_dev; a
 * stream may have zero frames in a chunk) and continues exactly where the previous chunk stopped, so that the rows of all
 * chunks together equal ONE wt_track_streams_dev call over the concatenated frames (tests/test_gpu_sort.py).
 *   out_frame     : frame index inside THIS chunk's CSR;
 *   out_local_id  : 0-based ordinal of the track's birth inside its stream (over all chunks).  The reference's object id
 *                   (process-global counter, sort.py:86,140-141) is id_base + births of the streams in front + ordinal + 1
 *                   and is known once those streams are complete: wt_track_global_ids_dev does that conversion for any
 *                   set of collected rows (row_stream = stream index of each row; stream_birth_prefix = n_streams + 1
 *                   int64 of device scratch, receives the exclusive prefix sum of births per stream).
 * max_frame_dets and params must be the same for every call on one state. */
size_t wt_track_state_bytes(int32_t n_streams, int64_t max_frame_dets, const wt_track_params* params);
int wt_track_state_init_dev(void* state, size_t state_bytes, int32_t n_streams, int64_t max_frame_dets,
                            const wt_track_params* params, void* stream);
size_t wt_track_chunk_workspace(int64_t n_dets, int64_t n_frames, int32_t n_streams, int64_t max_frame_dets,
                                const wt_track_params* params);
int wt_track_chunk_dev(void* state, size_t state_bytes,
                       int64_t n_dets, const double* x, const double* y, const double* w, const double* h,
                       const double* score, const int32_t* category,
                       int64_t n_frames, const int64_t* frame_det_offsets,
                       int32_t n_streams, const int64_t* stream_frame_offsets,
                       const double* clip_w, const double* clip_h, int64_t max_frame_dets,
                       const wt_track_params* params,
                       int64_t* out_frame, int32_t* out_category, double* out_bbox4, double* out_score,
                       int64_t* out_local_id, int64_t* n_out_dev, int64_t* n_births_dev,
                       void* workspace, size_t workspace_bytes, void* stream);
int wt_track_global_ids_dev(const void* state, size_t state_bytes, int32_t n_streams, int64_t max_frame_dets,
                            const wt_track_params* params, int64_t n_rows, const int32_t* row_stream,
                            const int64_t* local_id, int64_t id_base, int64_t* out_object_id,
                            int64_t* stream_birth_prefix, void* stream);

/* Native COCO-JSON I/O around the tracking stage (host code).
 * wt_detfile_read = json.load + read_data_file (tracking/utils.py:63-96: "annotations" wrapper, w/h < 1 and
 * per-class score filters, frame keys kept for fully filtered frames, missing score = 1.0) + the stream / frame
 * ordering of tracking/track.py:43-47 and utils.py:31, straight into the SoA / CSR layout of wt_track_streams_*.
 * The accessors return pointers owned by the handle (valid until wt_detfile_free). */
typedef struct wt_detfile wt_detfile;
int wt_detfile_read(const char* path, const double* score_threshold, int n_classes, wt_detfile** out);
void wt_detfile_free(wt_detfile* f);
int64_t wt_detfile_num_dets(const wt_detfile* f);
int64_t wt_detfile_num_frames(const wt_detfile* f);
int32_t wt_detfile_num_streams(const wt_detfile* f);
const double* wt_detfile_x(const wt_detfile* f);
const double* wt_detfile_y(const wt_detfile* f);
const double* wt_detfile_w(const wt_detfile* f);
const double* wt_detfile_h(const wt_detfile* f);
const double* wt_detfile_score(const wt_detfile* f);
const int32_t* wt_detfile_category(const wt_detfile* f);
const int64_t* wt_detfile_frame_det_offsets(const wt_detfile* f);
const int64_t* wt_detfile_stream_frame_offsets(const wt_detfile* f);
const int64_t* wt_detfile_frame_ids(const wt_detfile* f);
const char* wt_detfile_segment(const wt_detfile* f, int32_t stream);
const char* wt_detfile_camera(const wt_detfile* f, int32_t stream);
/* json.dump of the tracking rows (tracking/utils.py:52-58, tracking/track.py:50), byte-compatible with Python:
 * [{"image_id": "<segment>/<frame>/<camera>", "bbox": [x1, y1, w, h], "score": s, "category_id": c,
 *   "object_id": "<id>"}, ...]; floats in Python repr form.  Rows as produced by wt_track_streams_*. */
int wt_tracks_write_json(const char* path, const wt_detfile* f, int64_t n, const int64_t* frame, const int32_t* category,
                         const double* bbox4, const double* score, const int64_t* object_id);
/* Generic detection JSON = the wire format between inference, ensemble and tracking (detnet/data/coco.py:229-252,
 * detnet/ensemble.py:59-63,79,159-160): a list of {"image_id": str, "category_id": int, "bbox": [x, y, w, h], "score": float}.
 * wt_detjson_read = json.load of such a file into columns (image ids interned in first-appearance order; every entry must carry
 * the four keys, like convert_submission's det['score'] / det['bbox'] lookups, ensemble.py:35-45).
 * wt_detections_write_json = json.dump of rows whose boxes are integers (coco.py:250 int(v), ensemble.py:62 astype(int)) and whose
 * scores were rounded by the caller; key order image_id, category_id, bbox, score; strings escaped like json.dumps (ensure_ascii).
 * image ids: UTF-8 blob + (n_images + 1) offsets. */
typedef struct wt_detjson wt_detjson;
int wt_detjson_read(const char* path, wt_detjson** out);
void wt_detjson_free(wt_detjson* f);
int64_t wt_detjson_num_rows(const wt_detjson* f);
int32_t wt_detjson_num_images(const wt_detjson* f);
const int32_t* wt_detjson_image(const wt_detjson* f);
const int32_t* wt_detjson_category(const wt_detjson* f);
const double* wt_detjson_x(const wt_detjson* f);
const double* wt_detjson_y(const wt_detjson* f);
const double* wt_detjson_w(const wt_detjson* f);
const double* wt_detjson_h(const wt_detjson* f);
const double* wt_detjson_score(const wt_detjson* f);
const char* wt_detjson_image_id(const wt_detjson* f, int32_t i);
int wt_detections_write_json(const char* path, int64_t n, const int32_t* image_index, int32_t n_images, const char* image_id_blob,
                             const int64_t* image_id_offsets, const int32_t* category, const int64_t* bbox4, const double* score);
/* The same file for rows whose boxes are floats (detnet/ensemble_b.py:106-107 writes box.tolist() untruncated): every bbox value
 * in Python repr form, as json.dump writes a float. */
int wt_detections_write_json_f64(const char* path, int64_t n, const int32_t* image_index, int32_t n_images, const char* image_id_blob,
                                 const int64_t* image_id_offsets, const int32_t* category, const double* bbox4, const double* score);
/* Python repr() of a double (shortest round-trip digits); returns the length or -1 if cap is too small. */
int wt_format_double(double v, char* out, int cap);

/* =================================================================================================
 * soft-NMS / NMS / weighted-fusion ensemble
 * (detnet/utils/box_utils.py, detnet/nn/tta.py, detnet/ensemble.py)
 * ================================================================================================= */

/* nms(boxes, scores, overlap, top_k, soft=True, conf_thresh, soft_nms_cut) - detnet/utils/box_utils.py:307-395.
 * boxes4 (n,4) xyxy float64.  keep: kept indices in descending original-score order, out_scores: decayed
 * scores; both need n entries. */
int wt_softnms_f64_host(const double* boxes4, const double* scores, int n, double overlap, double cut,
                        double conf_thresh, int top_k, int64_t* keep, double* out_scores, int* n_keep);
/* Hard branch (detnet/utils/box_utils.py:329-333 -> torchvision.ops.nms): greedy, IoU > overlap suppresses. */
int wt_hardnms_f64_host(const double* boxes4, const double* scores, int n, double overlap, int top_k,
                        int64_t* keep, double* out_scores, int* n_keep);

/* ensemble(image_id, detections, category_ids) - detnet/ensemble.py:50-64 - for G (image,category) groups at
 * once: lxly2cxcy (:19-22) -> merge_func -> cxcy2lxly (:25-28).  Rows are [score,x_left,y_top,w,h] float64.
 *   method 0: merge_detections weighted fusion (detnet/nn/tta.py:22-66)
 *   method 1: nms_detections hard NMS          (detnet/nn/tta.py:8-19, soft=False)
 *   method 2: nms_detections linear soft-NMS   (detnet/nn/tta.py:8-19, soft=True, soft_nms_cut)
 *   method | 16: rows are [score,cx,cy,w,h] on input and output, i.e. the bare merge_func call signature of
 *                detnet/nn/tta.py:8,22 without the ensemble.py:19-28 conversions.
 * group_offsets (G+1) rows CSR; inside a group rows are the K inputs concatenated in input-file order and
 * input_sizes (G*K) gives the rows each input contributed (only method 0 reads it; may be NULL otherwise).
 * out5 has the input's row capacity: group g writes out_counts[g] rows starting at row group_offsets[g].
 * The min_score filter / astype(int) / round(score,5) of ensemble.py:59-62 is left to the caller. */
int wt_ensemble_groups_host(const double* dets5, const int64_t* group_offsets, const int32_t* input_sizes,
                            int64_t n_groups, int k_inputs, int method, double iou_thresh, double soft_nms_cut,
                            double* out5, int64_t* out_counts);
size_t wt_ensemble_groups_workspace(int64_t n_rows, int64_t n_groups, int64_t max_group_rows);
int wt_ensemble_groups_dev(const double* dets5, const int64_t* group_offsets, const int32_t* input_sizes,
                           int64_t n_rows, int64_t n_groups, int64_t max_group_rows, int k_inputs, int method,
                           double iou_thresh, double soft_nms_cut, double* out5, int64_t* out_counts,
                           void* workspace, size_t workspace_bytes, void* stream);

/* Ensemble of K test-time views of the same frames, slot to slot: the device form of exporting each view
 * (--tta V --export), detnet/ensemble.py over the K files and reading the result back as tracker slots.
 *   xywhs        : (K, 5, n_frames * slots) float64 wire rows [x, y, w, h, score] (integer boxes, 5-decimal scores)
 *   category     : (K, n_frames * slots) int32, 1..n_categories; 0 (or anything outside) = empty slot
 *   weights      : (K) float64 per-view weights (device)
 *   method       : 0 weighted fusion, 1 nms, 2 soft_nms
 * One (frame, category) group equals detnet/ensemble.py step for step: rows view by view in slot order, dropped unless
 * w > 0, h > 0 and score * weight >= min_score (:31-47); merged as wt_ensemble_groups_dev does with input_sizes = kept rows
 * per view (:50-58); kept if score > min_score, boxes truncated toward zero, score = numpy round(score, 5) (:59-63).
 *   out_xywhs    : (5, n_frames * K * slots), out_category (n_frames * K * slots): per frame the groups in ascending
 *                  category order, then empty slots (category 0, zero rows); out_counts (n_frames) int64 rows per frame.
 * Stream-ordered, no host synchronisation, no allocation: capturable in a hipGraph.  1 <= K <= 16. */
size_t wt_ensemble_slots_workspace(int64_t n_frames, int64_t slots, int k_views, int n_categories, int method);
int wt_ensemble_slots_dev(const double* xywhs, const int32_t* category, int64_t n_frames, int64_t slots, int k_views,
                          const double* weights, int n_categories, int method, double iou_thresh, double soft_nms_cut,
                          double min_score, double* out_xywhs, int32_t* out_category, int64_t* out_counts,
                          void* workspace, size_t workspace_bytes, void* stream);

/* Weighted boxes fusion and non-maximum weighted (the merge rules of detnet/ensemble_b.py) for G (image, category) groups at
 * once.  The definition is the project's own - DESIGN.md, "Weighted boxes fusion and NMW" - and is not pinned against the
 * ensemble_boxes package.  dets5 rows are [score, x_left, y_top, w, h] float64 with the score already multiplied by its input's
 * weight; group_offsets (G+1) rows CSR; inside a group the rows are the inputs concatenated in input order, each in file order.
 * group_wsum (G) float64: the weight sum of the inputs that have a row of any category in the group's image.
 *   method 0: weighted_fusion - rows in descending score (ties: earlier row) join the cluster whose fused box has the greatest
 *             IoU > iou_thresh (ties: earlier cluster) or start one; conf = mean score * min(wsum, members) / wsum
 *   method 1: nmw - the same walk against each cluster's first member; box weighted by score * IoU with it, conf = its score
 * out5 has the input's row capacity: group g writes out_counts[g] rows [conf, x_left, y_top, w, h] by descending conf (ties:
 * creation order) starting at row group_offsets[g]; out_members (rows, int32) holds the member count of each output row and
 * row_cluster (rows, int32) for each input row the position in its group's output of the cluster it joined; both may be NULL.
 * A group with more than max_group_rows rows is not merged: its out_counts is -1.
 * _dev: device pointers, stream-ordered, no allocation, no host synchronisation; workspace of wt_fuse_groups_workspace bytes
 * (0 while max_group_rows <= wt_fuse_groups_lds_rows(), the rows whose state fits the kernel's LDS).  An invalid method, a
 * negative size or a workspace that is too small is WT_ERR_INVALID. */
int64_t wt_fuse_groups_lds_rows(void);
size_t wt_fuse_groups_workspace(int64_t n_rows, int64_t n_groups, int64_t max_group_rows);
int wt_fuse_groups_dev(const double* dets5, const int64_t* group_offsets, const double* group_wsum, int64_t n_rows,
                       int64_t n_groups, int64_t max_group_rows, int method, double iou_thresh, double* out5,
                       int32_t* out_members, int32_t* row_cluster, int64_t* out_counts, void* workspace, size_t workspace_bytes,
                       void* stream);
int wt_fuse_groups_host(const double* dets5, const int64_t* group_offsets, const double* group_wsum, int64_t n_groups, int method,
                        double iou_thresh, double* out5, int32_t* out_members, int32_t* row_cluster, int64_t* out_counts);

/* Weighted boxes fusion / NMW of K test-time views of the same frames, slot to slot: the device form of exporting each view,
 * detnet/ensemble_b.py over the K files and reading the result back as tracker slots, between the pipeline's two score filters.
 * xywhs, category, weights, the outputs and the calling conventions are those of wt_ensemble_slots_dev; method is 0
 * (weighted_fusion) or 1 (nmw), the codes of wt_fuse_groups_*.  One (frame, category) group:
 *   rows view by view in slot order, kept when the category is in 1..n_categories, w > 0, h > 0 and score * weight >= min_score;
 *   a kept row's score is score * weight; wsum of the frame = the weights, added in view order, of the views that kept a row of
 *   ANY category in it; the group is merged as wt_fuse_groups_dev merges it; a cluster is kept if conf > min_score and leaves as
 *   [x1, y1, x2 - x1, y2 - y1] float64 (not truncated) with score = numpy round(conf, 5).
 * With min_score = -inf this is detnet/ensemble_b.py itself (whose CPython round differs from numpy's at decimal half-way points).
 *   out_xywhs (5, n_frames * K * slots), out_category, out_counts: per frame the groups in ascending category order, inside a
 *   group the clusters by descending conf (ties: creation order), then empty slots (category 0, zero rows).
 * Group state lives in LDS while K * slots <= wt_fuse_groups_lds_rows(), else in the workspace.  Stream-ordered, no host
 * synchronisation, no allocation: capturable in a hipGraph.  1 <= K <= 16.  Bad shapes, null pointers or a bad method are
 * WT_ERR_INVALID, a workspace below wt_fuse_slots_workspace bytes WT_ERR_CAPACITY, both before any launch; the sizer returns 0
 * for a bad shape. */
size_t wt_fuse_slots_workspace(int64_t n_frames, int64_t slots, int k_views, int n_categories, int method);
int wt_fuse_slots_dev(const double* xywhs, const int32_t* category, int64_t n_frames, int64_t slots, int k_views,
                      const double* weights, int n_categories, int method, double iou_thresh, double min_score,
                      double* out_xywhs, int32_t* out_category, int64_t* out_counts,
                      void* workspace, size_t workspace_bytes, void* stream);

/* =================================================================================================
 * MOT evaluation (CLEAR-MOT per class and Waymo difficulty level; the definition is in DESIGN.md, "Tracking metric")
 * ================================================================================================= */

/* Scores K >= 1 tracking results against one ground truth: one wavefront per (result set, stream, class) walks the stream's
 * frames in order (carry last frame's pairs that still reach the class's IoU threshold, assign the rest with the
 * linear_assignment of tracking/sort/sort.py:206 on the gated float32 IoU matrix, count).  IoU is float64 on [x, y, x+w, y+h]
 * in the operation order of tracking/sort/sort.py:34-47.
 *
 * Ground truth: SoA rows sorted by (stream, frame, file order) - x, y, w, h float64, category int32 (rows outside
 * 1..n_classes are skipped), level int32 (2 = LEVEL_2 only, anything else counts at both levels), gt_id int32 = object id
 * interned per stream to 0..max_gt_ids-1 - with the CSR offsets frame_gt_offsets (n_frames + 1) and stream_frame_offsets
 * (n_streams + 1); the frames of a stream ascend.  An id occurs at most once per frame.
 * Results: the K sets concatenated; set k owns rows set_row_offsets[k] .. set_row_offsets[k + 1] and lists first the rows on
 * the ground truth's frames, sorted like the ground truth, with frame_hyp_offsets[k * (n_frames + 1) + f] their offsets inside
 * the set, then the rows that take no part (other frames, unknown streams).  h_id int32 >= 0 = object id interned per (set,
 * stream); an id occurs at most once per frame and class.
 * thr: n_classes <= 16 IoU thresholds, host pointer, read before the call returns.
 * max_frame_boxes: upper bound of the boxes of ONE class in one frame on either side (<= 4096, more is WT_ERR_CAPACITY).
 * Outputs: counts (K, n_streams, n_classes, 2, 5) int64 = gt, tp, fn, fp, idsw for LEVEL_1, LEVEL_2;
 *          iou_sum (K, n_streams, n_classes, 2) float64, summed in frame order, then ground-truth row order;
 *          hyp_match (per result row, may be NULL): matched ground-truth row, -1 false positive, -2 took no part;
 *          hyp_switch (per result row, may be NULL): 1 where the match is an identity switch.
 * The device form also reports in status_dev (device int32) 0 or the WT_ERR_* a wavefront met (capacity, assignment did
 * not converge); it does not check the layout, the host form does (WT_ERR_INVALID names the frame). */
size_t wt_mot_eval_workspace(int32_t k_sets, int32_t n_streams, int32_t n_classes, int64_t max_frame_boxes, int32_t max_gt_ids);
int wt_mot_eval_dev(int64_t n_gt, const double* gx, const double* gy, const double* gw, const double* gh,
                    const int32_t* g_category, const int32_t* g_level, const int32_t* g_id,
                    int64_t n_frames, const int64_t* frame_gt_offsets, int32_t n_streams, const int64_t* stream_frame_offsets,
                    int32_t k_sets, int64_t n_hyp, const int64_t* set_row_offsets, const int64_t* frame_hyp_offsets,
                    const double* hx, const double* hy, const double* hw, const double* hh,
                    const int32_t* h_category, const int32_t* h_id,
                    int32_t n_classes, const double* thr, int64_t max_frame_boxes, int32_t max_gt_ids,
                    int64_t* counts, double* iou_sum, int64_t* hyp_match, uint8_t* hyp_switch, int32_t* status_dev,
                    void* workspace, size_t workspace_bytes, void* stream);
int wt_mot_eval_host(int64_t n_gt, const double* gx, const double* gy, const double* gw, const double* gh,
                     const int32_t* g_category, const int32_t* g_level, const int32_t* g_id,
                     int64_t n_frames, const int64_t* frame_gt_offsets, int32_t n_streams, const int64_t* stream_frame_offsets,
                     int32_t k_sets, const int64_t* set_row_offsets, const int64_t* frame_hyp_offsets,
                     const double* hx, const double* hy, const double* hw, const double* hh,
                     const int32_t* h_category, const int32_t* h_id,
                     int32_t n_classes, const double* thr,
                     int64_t* counts, double* iou_sum, int64_t* hyp_match, uint8_t* hyp_switch);

/* =================================================================================================
 * MOT identity evaluation (IDF1 / IDP / IDR per class and Waymo difficulty level; the definition is DESIGN.md section 18)
 * ================================================================================================= */

/* Scores the identity preservation of K >= 1 tracking results against one ground truth: one wavefront per (result set,
 * stream, class) walks the stream's frames in order and counts, per (ground-truth trajectory, hypothesis trajectory), the
 * frames where both have a box and IoU >= the class's threshold (one float32 matrix per difficulty level, the smaller side as
 * rows), solves ONE assignment per level on that matrix (the Munkres of the tracker, on -n) and walks the frames once more to
 * count the pairs whose trajectories are assigned to each other.  IoU as in wt_mot_eval_*.
 *
 * Ground truth and results: the SoA layout of wt_mot_eval_* unchanged (the same arrays can be passed), except that the object
 * ids are replaced by trajectory indices: g_traj int32 = index of the row's trajectory among those of its (stream, class),
 * h_traj int32 = the same among those of its (set, stream, class); rows of other categories and rows that take no part are not
 * read.  A trajectory occurs at most once per frame.  g_ntraj (n_streams, n_classes) and h_ntraj (K, n_streams, n_classes)
 * int32 are the trajectory counts (each <= 4096, more is WT_ERR_CAPACITY).
 * mat_offsets (K * n_streams * n_classes + 1) int64, device form only: where each problem's two matrices start inside the
 * matrix part of the workspace, in floats; problem p needs 2 * min(g, h) * (max(g, h) | 1) floats, matrix_floats =
 * mat_offsets[last] is the total.  The host form computes them.
 * max_gt_traj / max_hyp_traj: upper bounds of g_ntraj / h_ntraj (size the per-wavefront scratch).
 * Outputs: id_counts (K, n_streams, n_classes, 2, 3) int64 = idtp, gt, hyp for LEVEL_1, LEVEL_2;
 *          hyp_idmatch (n_hyp, 2) int64, may be NULL: per result row and level the ground-truth row the box is
 *          identity-matched to, -1 not matched, -2 took no part or is left out at that level.  The matching behind it is ONE
 *          optimal assignment; idtp does not depend on which.
 * The device form takes device pointers (thr: host pointer, read before the call returns), is stream-ordered, never allocates
 * or synchronises, and reports in status_dev (device int32) 0 or the WT_ERR_* a wavefront met (capacity: counts or offsets
 * that do not fit the rows; assignment did not converge), after which that wavefront's outputs stay zero.  A workspace smaller
 * than wt_mot_identity_workspace() says is WT_ERR_INVALID and nothing is launched.  It does not check the layout; the host form
 * does (WT_ERR_INVALID names the frame), stages everything itself, and fails with WT_ERR_INVALID when the workspace it needs
 * exceeds workspace_limit_bytes (0 = no limit): the caller then scores fewer results per call.
 * wt_mot_identity_limits: 4096, and the sizes up to which the star arrays (2 min + max ints) and the zero bitmaps
 * (min * ceil(max / 64) * 8 bytes) of the largest problem stay in LDS; beyond them they live in the workspace. */
void wt_mot_identity_limits(int32_t* max_trajectories, int64_t* lds_stars_bytes, int64_t* lds_zmask_bytes);
size_t wt_mot_identity_workspace(int32_t k_sets, int32_t n_streams, int32_t n_classes, int64_t max_gt_traj, int64_t max_hyp_traj,
                                 int64_t matrix_floats);
int wt_mot_identity_dev(int64_t n_gt, const double* gx, const double* gy, const double* gw, const double* gh,
                        const int32_t* g_category, const int32_t* g_level, const int32_t* g_traj,
                        int64_t n_frames, const int64_t* frame_gt_offsets, int32_t n_streams, const int64_t* stream_frame_offsets,
                        int32_t k_sets, int64_t n_hyp, const int64_t* set_row_offsets, const int64_t* frame_hyp_offsets,
                        const double* hx, const double* hy, const double* hw, const double* hh,
                        const int32_t* h_category, const int32_t* h_traj,
                        const int32_t* g_ntraj, const int32_t* h_ntraj, const int64_t* mat_offsets, int64_t matrix_floats,
                        int32_t n_classes, const double* thr, int64_t max_gt_traj, int64_t max_hyp_traj,
                        int64_t* id_counts, int64_t* hyp_idmatch, int32_t* status_dev,
                        void* workspace, size_t workspace_bytes, void* stream);
int wt_mot_identity_host(int64_t n_gt, const double* gx, const double* gy, const double* gw, const double* gh,
                         const int32_t* g_category, const int32_t* g_level, const int32_t* g_traj,
                         int64_t n_frames, const int64_t* frame_gt_offsets, int32_t n_streams, const int64_t* stream_frame_offsets,
                         int32_t k_sets, const int64_t* set_row_offsets, const int64_t* frame_hyp_offsets,
                         const double* hx, const double* hy, const double* hw, const double* hh,
                         const int32_t* h_category, const int32_t* h_traj,
                         const int32_t* g_ntraj, const int32_t* h_ntraj,
                         int32_t n_classes, const double* thr, size_t workspace_limit_bytes,
                         int64_t* id_counts, int64_t* hyp_idmatch);

/* =================================================================================================
 * MOT HOTA evaluation (HOTA / DetA / AssA / LocA per class and Waymo difficulty level; the definition is DESIGN.md section 19)
 * ================================================================================================= */

/* Scores K >= 1 tracking results against one ground truth with HOTA (Luiten et al. 2021) at the 19 localisation thresholds
 * alpha_a = (a + 1) / 20: one wavefront per (result set, stream, class, difficulty level) walks the stream's frames twice.  The
 * first walk adds, per (ground-truth trajectory, hypothesis trajectory), the frame's S / (row + col - S) of every overlapping
 * pair into a float64 matrix and turns it into the alignment score A = P / (cg + ch - P); the second solves ONE assignment per
 * frame on the float32 matrix A * IoU (the Munkres of the tracker on its negative, no gate) and counts every kept pair at the
 * thresholds its IoU reaches.  LEVEL_1 is the same computation without the level-2 ground-truth rows and without the result rows
 * that, in their frame, reach the class's thr with a removed row and with no counted one; thr has no other use.  IoU as in
 * wt_mot_eval_*.
 *
 * Ground truth, results, trajectory indices and counts: exactly the arguments of wt_mot_identity_*.
 * mat_offsets (K * n_streams * n_classes + 1) int64, device form only: where each problem's cells start inside the matrix part
 * of the workspace; problem p needs 2 * g_ntraj * h_ntraj cells (one matrix per level), matrix_cells = mat_offsets[last] is the
 * total.  A cell is 46 bytes: the float64 score and 19 uint16 match counts.  The host form computes the offsets.
 * max_frame_boxes: upper bound of the boxes of ONE class in one frame on either side (<= 4096, more is WT_ERR_CAPACITY);
 * max_gt_traj / max_hyp_traj: upper bounds of g_ntraj / h_ntraj (<= 4096 likewise).  A stream has at most 65535 frames.
 * Outputs: hota_counts (K, n_streams, n_classes, 2, 21) int64 = gt, hyp, tp[19] for LEVEL_1, LEVEL_2;
 *          hota_sums (K, n_streams, n_classes, 2, 19, 4) float64 = ass, assre, asspr, loc per threshold; loc is added in frame
 *          order, then ground-truth row order; the association sums are added per lane over the cells l, l + 64, ... and then
 *          over the lanes in order, the same on every run;
 *          hyp_match (n_hyp, 2) int64, may be NULL: per result row and level the ground-truth row the frame's assignment
 *          gave it, -1 unmatched, -2 took no part or was removed at that level.  It does not depend on the threshold.
 * The device form takes device pointers (thr: host pointer, read before the call returns), is stream-ordered, never allocates
 * or synchronises, and reports in status_dev (device int32) 0 or the WT_ERR_* a wavefront met (capacity: counts or offsets that
 * do not fit the rows; assignment did not converge), after which that wavefront's outputs stay zero.  A workspace smaller than
 * wt_mot_hota_workspace() says is WT_ERR_INVALID and nothing is launched.  It does not check the layout; the host form does
 * (WT_ERR_INVALID names the frame), stages everything itself, and fails with WT_ERR_INVALID when the workspace it needs exceeds
 * workspace_limit_bytes (0 = no limit): the caller then scores fewer results per call.
 * wt_mot_hota_limits: 4096, 4096, 65535, and the sizes up to which a frame's cost matrix (min * (max | 1) floats) and its zero
 * bitmaps (n * ceil(n / 64) * 8 bytes at max_frame_boxes = n) stay in LDS; beyond them they live in the workspace. */
void wt_mot_hota_limits(int32_t* max_frame_boxes, int32_t* max_trajectories, int32_t* max_stream_frames, int64_t* lds_cost_floats,
                        int64_t* lds_zmask_bytes);
size_t wt_mot_hota_workspace(int32_t k_sets, int32_t n_streams, int32_t n_classes, int64_t max_frame_boxes, int64_t max_gt_traj,
                             int64_t max_hyp_traj, int64_t matrix_cells);
int wt_mot_hota_dev(int64_t n_gt, const double* gx, const double* gy, const double* gw, const double* gh,
                    const int32_t* g_category, const int32_t* g_level, const int32_t* g_traj,
                    int64_t n_frames, const int64_t* frame_gt_offsets, int32_t n_streams, const int64_t* stream_frame_offsets,
                    int32_t k_sets, int64_t n_hyp, const int64_t* set_row_offsets, const int64_t* frame_hyp_offsets,
                    const double* hx, const double* hy, const double* hw, const double* hh,
                    const int32_t* h_category, const int32_t* h_traj,
                    const int32_t* g_ntraj, const int32_t* h_ntraj, const int64_t* mat_offsets, int64_t matrix_cells,
                    int32_t n_classes, const double* thr, int64_t max_frame_boxes, int64_t max_gt_traj, int64_t max_hyp_traj,
                    int64_t* hota_counts, double* hota_sums, int64_t* hyp_match, int32_t* status_dev,
                    void* workspace, size_t workspace_bytes, void* stream);
int wt_mot_hota_host(int64_t n_gt, const double* gx, const double* gy, const double* gw, const double* gh,
                     const int32_t* g_category, const int32_t* g_level, const int32_t* g_traj,
                     int64_t n_frames, const int64_t* frame_gt_offsets, int32_t n_streams, const int64_t* stream_frame_offsets,
                     int32_t k_sets, const int64_t* set_row_offsets, const int64_t* frame_hyp_offsets,
                     const double* hx, const double* hy, const double* hw, const double* hh,
                     const int32_t* h_category, const int32_t* h_traj,
                     const int32_t* g_ntraj, const int32_t* h_ntraj,
                     int32_t n_classes, const double* thr, size_t workspace_limit_bytes,
                     int64_t* hota_counts, double* hota_sums, int64_t* hyp_match);

/* =================================================================================================
 * MOT trajectory coverage (MT / PT / ML and fragmentations per class and Waymo difficulty level; the definition is DESIGN.md
 * section 27)
 * ================================================================================================= */

/* Says what happened to every ground-truth trajectory under the matching of wt_mot_eval_*: a consumer of the hyp_match and
 * hyp_switch that call leaves behind, integers only.  Three passes on one stream: a mark pass (one lane per result row writes one
 * byte at (set, matched ground-truth row)), a link pass (one wavefront per (stream, class), once per call, chains every
 * ground-truth row to the next row of its trajectory) and a walk pass (one lane per (result set, trajectory) follows its chain).
 * At LEVEL_1 the rows with level 2 do not exist; a trajectory without a row at a level is none at that level.  Per trajectory
 * and level: len rows, tracked of them matched, frag = runs of unmatched rows with a matched row before and after, idsw =
 * matched rows whose match is an identity switch.  Mostly tracked: 5 * tracked >= 4 * len; mostly lost: 5 * tracked < len;
 * partially tracked otherwise.
 *
 * Ground truth: g_category, g_level, frame_gt_offsets, stream_frame_offsets as wt_mot_eval_* takes them; g_traj and g_ntraj
 * (n_streams, n_classes) as wt_mot_identity_* takes them (each count <= 4096, a stream has at most 65535 frames; more is
 * WT_ERR_CAPACITY); traj_offsets (n_streams * n_classes + 1) int64 = the exclusive scan of g_ntraj, total_traj its last entry: the
 * trajectories of all (stream, class) are numbered in that order.
 * Results: k_sets, n_hyp, set_row_offsets as wt_mot_eval_dev takes them, and its outputs hyp_match and hyp_switch (n_hyp each).
 * Outputs: cov_counts (K, n_streams, n_classes, 2, 5) int64 = traj, mt, pt, ml, frag for LEVEL_1, LEVEL_2;
 *          traj_stats (K, total_traj, 2, 4) int32 = len, tracked, frag, idsw for LEVEL_1, LEVEL_2, may be NULL (16-byte aligned).
 * The device form takes device pointers, is stream-ordered, never allocates or synchronises, clears what it reads inside the
 * call, and reports in status_dev (device int32) 0 or WT_ERR_CAPACITY (counts, offsets, trajectory indices or matches that do not
 * fit the rows), after which that (stream, class)'s outputs stay zero.  A workspace smaller than wt_mot_coverage_workspace() says
 * is WT_ERR_INVALID and nothing is launched.  pass_events: NULL, or four hipEvent_t the call records before the clears and after
 * each pass (for measurements).  It does not check the layout; the host form does (WT_ERR_INVALID names the frame).
 * The host form takes the arguments of wt_mot_eval_host (g_id / h_id are object ids) and the trajectory columns beside them,
 * stages everything itself and runs wt_mot_eval_dev and the three passes on one stream. */
size_t wt_mot_coverage_workspace(int32_t k_sets, int32_t n_streams, int32_t n_classes, int64_t n_gt, int64_t total_traj);
int wt_mot_coverage_dev(int64_t n_gt, const int32_t* g_category, const int32_t* g_level, const int32_t* g_traj,
                        int64_t n_frames, const int64_t* frame_gt_offsets, int32_t n_streams, const int64_t* stream_frame_offsets,
                        int32_t n_classes, const int32_t* g_ntraj, const int64_t* traj_offsets, int64_t total_traj,
                        int32_t k_sets, int64_t n_hyp, const int64_t* set_row_offsets, const int64_t* hyp_match, const uint8_t* hyp_switch,
                        int64_t* cov_counts, int32_t* traj_stats, int32_t* status_dev,
                        void* workspace, size_t workspace_bytes, void* stream, void* const* pass_events);
int wt_mot_coverage_host(int64_t n_gt, const double* gx, const double* gy, const double* gw, const double* gh,
                         const int32_t* g_category, const int32_t* g_level, const int32_t* g_id, const int32_t* g_traj,
                         int64_t n_frames, const int64_t* frame_gt_offsets, int32_t n_streams, const int64_t* stream_frame_offsets,
                         int32_t k_sets, const int64_t* set_row_offsets, const int64_t* frame_hyp_offsets,
                         const double* hx, const double* hy, const double* hw, const double* hh,
                         const int32_t* h_category, const int32_t* h_id,
                         const int32_t* g_ntraj, int32_t n_classes, const double* thr,
                         int64_t* cov_counts, int32_t* traj_stats);

/* =================================================================================================
 * Track refinement (length filter, linear gap filling, mean track score; the definition is DESIGN.md section 20)
 * ================================================================================================= */

/* Refines R >= 1 tracking results under J jobs: job j names a result, job_result[j], and its parameters, and yields a result of
 * its own.  One wavefront per (job, stream) walks the stream's frame slots twice: the first walk links every row to the next
 * observation of its trajectory and counts, the second emits.  A trajectory = the rows of one (result, stream) with the same
 * local index; its class is the category of its first observation.  A trajectory with fewer than min_len[class] observations is
 * removed; between two consecutive observations n slots apart, 2 <= n <= max_gap[class] + 1, one row is added at each slot in
 * between with x, y, w, h, score = va + (vb - va) * ((double)j / (double)n), every operation rounded on its own in float64, and
 * the category of the earlier one; with score_mode 1 every row of a trajectory carries the mean of its observed scores, added
 * one by one in slot order and divided by their count (0: observed rows keep theirs).
 *
 * Results: the R sets concatenated, SoA - x, y, w, h, score float64, category int32 in 1..n_classes, local int32 = the row's
 * trajectory numbered densely per (result, stream) - set r owning rows set_row_offsets[r] .. set_row_offsets[r + 1], sorted by
 * frame slot, with frame_row_offsets[r * (n_frames + 1) + f] their offsets inside the set (rows behind the last offset take no
 * part) and stream_frame_offsets (n_streams + 1) the slots of each stream.  A trajectory occurs at most once per slot.
 * The host form takes n_traj (R, n_streams) int32, the trajectory counts; the device forms take their running sum traj_offsets
 * (R * n_streams + 1) int64 with n_traj_total = its last entry and max_traj = an upper bound of the counts.
 * Jobs: job_result (J) int32, job_max_gap and job_min_len (J, n_classes) int32 (>= 0 and >= 1), job_score_mode (J) int32.
 * Outputs, job after job, inside a job slot after slot, inside a slot the surviving input rows in input order, then the added
 * rows in ascending local index: out_frame int64 (slot), out_category, out_bbox (n, 4) = x, y, w, h, out_score, out_local,
 * out_source int64 = the row's index inside its result, or -1 - (index of the gap's later observation) for an added row;
 * job_row_offsets (J + 1) int64 = the rows of each job; out_frame_row_offsets (J, n_frames + 1) int64 = the slot offsets inside
 * each job, the frame_hyp_offsets wt_mot_*_dev takes.  max_gap 0, min_len 1, score_mode 0 reproduces the input.
 *
 * wt_refine_tracks_plan_dev links, counts and scans: device pointers, stream-ordered, no allocation, no synchronisation; it
 * writes job_row_offsets (device) and reports in status_dev (device int32) 0 or WT_ERR_CAPACITY (counts, indices or offsets that
 * do not fit the rows).  wt_refine_tracks_emit_dev writes the rows, given the same arguments and the workspace the plan left; it
 * waits for the stream once, to read the planned size: out_cap below it is WT_ERR_CAPACITY and nothing is launched.  A workspace
 * smaller than wt_refine_tracks_workspace() says is WT_ERR_INVALID.  The device forms do not check the layout; the host form does
 * (WT_ERR_INVALID names the result and the row or frame slot), stages, plans and emits; with out_cap = 0 it only plans and
 * returns job_row_offsets (the output pointers may then be NULL): the sizing call.
 * wt_refine_tracks_limits: the trajectory count of one (result, stream) up to which the per-trajectory tables stay in LDS;
 * above it they live in the workspace. */
void wt_refine_tracks_limits(int32_t* lds_trajectories);
size_t wt_refine_tracks_workspace(int32_t n_jobs, int32_t n_streams, int64_t n_rows, int64_t n_traj_total, int64_t max_traj);
int wt_refine_tracks_plan_dev(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                              int32_t r_sets, int64_t n_rows, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                              const double* score, const int32_t* category, const int32_t* local,
                              const int64_t* traj_offsets, int64_t n_traj_total, int64_t max_traj,
                              int32_t n_jobs, const int32_t* job_result, const int32_t* job_max_gap, const int32_t* job_min_len, int32_t n_classes,
                              int64_t* job_row_offsets, int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream);
int wt_refine_tracks_emit_dev(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                              int32_t r_sets, int64_t n_rows, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                              const double* x, const double* y, const double* w, const double* h, const double* score,
                              const int32_t* category, const int32_t* local,
                              const int64_t* traj_offsets, int64_t n_traj_total, int64_t max_traj,
                              int32_t n_jobs, const int32_t* job_result, const int32_t* job_max_gap, const int32_t* job_min_len,
                              const int32_t* job_score_mode, int32_t n_classes, const int64_t* job_row_offsets, int64_t out_cap,
                              int64_t* out_frame, int32_t* out_category, double* out_bbox, double* out_score, int32_t* out_local,
                              int64_t* out_source, int64_t* out_frame_row_offsets,
                              int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream);
int wt_refine_tracks_host(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                          int32_t r_sets, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                          const double* x, const double* y, const double* w, const double* h, const double* score,
                          const int32_t* category, const int32_t* local, const int32_t* n_traj,
                          int32_t n_jobs, const int32_t* job_result, const int32_t* job_max_gap, const int32_t* job_min_len,
                          const int32_t* job_score_mode, int32_t n_classes, int64_t out_cap,
                          int64_t* out_frame, int32_t* out_category, double* out_bbox, double* out_score, int32_t* out_local,
                          int64_t* out_source, int64_t* out_frame_row_offsets, int64_t* job_row_offsets);

/* =================================================================================================
 * Track stitching (the second association pass: tracklets linked across gaps; the definition is DESIGN.md section 21)
 * ================================================================================================= */

/* Stitches R >= 1 tracking results under J jobs: job j names a result, job_result[j], and its parameters.  Results, trajectories
 * and local indices are those of the track refinement above, with one more requirement: the local indices of a (result, stream)
 * number its trajectories by first appearance, none missing.  Tail i (last observation at slot e, box x, y, w, h; the one before
 * at slot p) and head j of the same stream and class (first observation at slot s) are a candidate when n = s - e lies in
 * 1..max_link[class] and the affinity a satisfies a >= link_iou[class] and a > 0 (a NaN never does).  a = iou_dd of
 * [px, py, px + w, py + h] and the head's first box, with px = x + ((x - x_p) / (double)(e - p)) * (double)n, py alike, when
 * motion is 1 (linear) and the tail has two observations, and px = x, py = y otherwise (motion 0 = hold); every operation rounded
 * on its own in float64.  The candidates are walked in the strict order (-a, n, i, j) and one is accepted when i is not yet a tail
 * and j not yet a head: the links form chains, and every row takes the identity of its chain's earliest trajectory (the root).
 *
 * Jobs: job_result (J) int32, job_max_link (J, n_classes) int32 >= 0 (0: the class is never linked), job_link_iou (J, n_classes)
 * float64 not NaN, job_motion (J) int32.
 * Outputs, sized up front: out_pred, out_root (J, n_traj_total) int32 and out_affinity (J, n_traj_total) float64, indexed like
 * traj_offsets - the local index linked into the trajectory or -1, its root's local index, the accepted link's a or -1.0;
 * out_row_root (J, n_rows) int32 = per row of the job's result the root's local index; out_links (J, n_streams) int64 = the links
 * made.  Entries of results the job does not name are -1 (-1.0).  A job whose max_link is all 0 has pred -1 and root = the index.
 *
 * wt_stitch_tracks_dev: device pointers, stream-ordered, no allocation, no synchronisation; it reports in status_dev (device
 * int32) 0 or WT_ERR_CAPACITY (counts, indices or offsets that do not fit the rows).  A workspace smaller than
 * wt_stitch_tracks_workspace() says is WT_ERR_CAPACITY.  The device form does not check the layout; the host form does
 * (WT_ERR_INVALID names the result and the row or frame slot, or the job), stages and launches; it takes n_traj (R, n_streams)
 * int32 where the device form takes the running sum traj_offsets, n_traj_total and max_traj.
 * wt_stitch_tracks_limits: the trajectory count of one (result, stream) up to which the tables of the matching stay in LDS;
 * above it they live in the workspace. */
void wt_stitch_tracks_limits(int32_t* lds_trajectories);
size_t wt_stitch_tracks_workspace(int32_t n_jobs, int32_t n_streams, int64_t n_rows, int64_t n_traj_total, int64_t max_traj);
int wt_stitch_tracks_dev(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                         int32_t r_sets, int64_t n_rows, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                         const double* x, const double* y, const double* w, const double* h, const int32_t* category, const int32_t* local,
                         const int64_t* traj_offsets, int64_t n_traj_total, int64_t max_traj,
                         int32_t n_jobs, const int32_t* job_result, const int32_t* job_max_link, const double* job_link_iou,
                         const int32_t* job_motion, int32_t n_classes,
                         int32_t* out_pred, int32_t* out_root, double* out_affinity, int32_t* out_row_root, int64_t* out_links,
                         int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream);
int wt_stitch_tracks_host(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                          int32_t r_sets, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                          const double* x, const double* y, const double* w, const double* h, const int32_t* category, const int32_t* local,
                          const int32_t* n_traj, int32_t n_jobs, const int32_t* job_result, const int32_t* job_max_link,
                          const double* job_link_iou, const int32_t* job_motion, int32_t n_classes,
                          int32_t* out_pred, int32_t* out_root, double* out_affinity, int32_t* out_row_root, int64_t* out_links);

/* =================================================================================================
 * Track splitting (impure tracks cut at motion jumps and long gaps; the definition is DESIGN.md section 25)
 * ================================================================================================= */

/* Splits the trajectories of R >= 1 tracking results under J jobs: job j names a result, job_result[j], and its parameters.
 * Results, frame slots, streams, trajectories, local indices (in any order) and a trajectory's class are those of the track
 * refinement above.  A trajectory has its observations at slots f_0 < f_1 < ...; the pair (i - 1, i), n = f_i - f_{i-1}, breaks
 * when split_gap[class] > 0 and n > split_gap[class], or - when split_iou[class] > 0 - when every test that exists for it gives
 * a < split_iou[class] (a NaN never does):
 *   forward  (motion 1 = linear and i >= 2):     p = f_{i-1} - f_{i-2}, px = x_{i-1} + ((x_{i-1} - x_{i-2}) / (double)p) * (double)n, py
 *            alike, w and h of row i - 1; a_f = iou_dd([px, py, px + w, py + h], box_i);
 *   backward (motion 1 and row i + 1 exists):    q = f_{i+1} - f_i, px = x_i + ((x_i - x_{i+1}) / (double)q) * (double)n, py alike,
 *            w and h of row i; a_b = iou_dd([px, py, px + w, py + h], box_{i-1});
 *   hold     (neither exists; motion 0 = hold):  a_h = iou_dd(box_{i-1}, box_i);
 * every operation rounded on its own in float64.  piece(row) = the breaking pairs of its trajectory at or before the row; piece 0
 * keeps the identity, and the other pieces of a result are numbered from 0 in the order (stream, local index, piece).
 *
 * Jobs: job_result (J) int32, job_split_iou (J, n_classes) float64 not NaN (<= 0: the rule is off for the class), job_split_gap
 * (J, n_classes) int32 >= 0 (0: off), job_motion (J) int32.
 * Outputs, sized up front: out_piece (J, n_rows) int32; out_new (J, n_rows) int64 = the number of the row's new piece, -1 for
 * piece 0 (the caller gives the row the id first_new_id + out_new); out_test (J, n_rows, 2) float64 = for the pair that ends at
 * the row [a_f, or a_h when the hold test was used, or -1.0; a_b or -1.0], both -1.0 for a trajectory's first row and when the
 * class's IoU rule is off; out_breaks (J, n_traj_total) int32, indexed like traj_offsets; out_new_pieces (J, n_streams) int64 =
 * the breaks of the stream.  Entries of results the job does not name are -1 (-1.0).
 *
 * wt_split_tracks_dev: device pointers, stream-ordered, no allocation, no synchronisation; it reports in status_dev (device
 * int32) 0 or WT_ERR_CAPACITY (counts, indices or offsets that do not fit the rows).  A workspace smaller than
 * wt_split_tracks_workspace() says is WT_ERR_CAPACITY.  The device form does not check the layout; the host form does
 * (WT_ERR_INVALID names the result and the row or frame slot, or the job and class), stages and launches; it takes n_traj
 * (R, n_streams) int32 where the device form takes the running sum traj_offsets, n_traj_total and max_traj.
 * wt_split_tracks_limits: the trajectory count of one (result, stream) up to which the per-trajectory tables stay in LDS; above
 * it they live in the workspace. */
void wt_split_tracks_limits(int32_t* lds_trajectories);
size_t wt_split_tracks_workspace(int32_t n_jobs, int32_t n_streams, int64_t n_rows, int64_t n_traj_total, int64_t max_traj);
int wt_split_tracks_dev(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                        int32_t r_sets, int64_t n_rows, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                        const double* x, const double* y, const double* w, const double* h, const int32_t* category, const int32_t* local,
                        const int64_t* traj_offsets, int64_t n_traj_total, int64_t max_traj,
                        int32_t n_jobs, const int32_t* job_result, const double* job_split_iou, const int32_t* job_split_gap,
                        const int32_t* job_motion, int32_t n_classes,
                        int32_t* out_piece, int64_t* out_new, double* out_test, int32_t* out_breaks, int64_t* out_new_pieces,
                        int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream);
int wt_split_tracks_host(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                         int32_t r_sets, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                         const double* x, const double* y, const double* w, const double* h, const int32_t* category, const int32_t* local,
                         const int32_t* n_traj, int32_t n_jobs, const int32_t* job_result, const double* job_split_iou,
                         const int32_t* job_split_gap, const int32_t* job_motion, int32_t n_classes,
                         int32_t* out_piece, int64_t* out_new, double* out_test, int32_t* out_breaks, int64_t* out_new_pieces);

/* =================================================================================================
 * Track smoothing (a symmetric window filter per trajectory; the definition is DESIGN.md section 22)
 * ================================================================================================= */

#define WT_SMOOTH_MAX_WINDOW 32

/* Smooths the boxes of R >= 1 tracking results under J jobs: job j names a result, job_result[j], a window per class and a weight
 * table per class.  Results, frame slots, streams, trajectories, local indices and a trajectory's class (the category of its first
 * observation) are those of the track refinement above.  For the row of trajectory T at slot f, W = window[class], k = the
 * class's weights, and each of x, y, w, h on its own:
 *     acc = k[0] * v(f), den = k[0]; for d = 1 .. W ascending, only when T has a row at slot f - d AND one at slot f + d:
 *     acc = acc + k[d] * (v(f - d) + v(f + d)), den = den + (k[d] + k[d]); out = acc / den,
 * every operation rounded on its own in float64, all reads from the input.  A row that no pair contributed to keeps its input
 * bits.  No row is added, removed or moved; score, category and identity are not read or written.
 *
 * Jobs: job_result (J) int32, job_window (J, n_classes) int32 in 0..WT_SMOOTH_MAX_WINDOW (0: the class is untouched),
 * job_weights (J, n_classes, n_weights) float64, finite, >= 0, [..][0] > 0, n_weights > every window.
 * Outputs: job after job, each job owning the rows of its result in the result's row order: job_row_offsets (J + 1) int64 is the
 * running sum of those row counts, computed by the caller, and n_out_rows its last entry.  out_bbox (n_out_rows, 4) float64 =
 * x, y, w, h; out_pairs (n_out_rows) int32 = the pairs that contributed to the row.
 *
 * wt_smooth_tracks_dev: device pointers, stream-ordered, no allocation, no synchronisation; it reports in status_dev (device
 * int32) 0 or WT_ERR_CAPACITY (counts, indices, offsets or windows that do not fit).  A workspace smaller than
 * wt_smooth_tracks_workspace() says is WT_ERR_CAPACITY.  The device form does not check the layout; the host form does
 * (WT_ERR_INVALID names the result and the row or frame slot, or the job), computes job_row_offsets, stages and launches; it takes
 * n_traj (R, n_streams) int32 where the device form takes the running sum traj_offsets, n_traj_total and max_traj.
 * wt_smooth_tracks_limits: the trajectory count of one (result, stream) up to which the table of the link walk stays in LDS;
 * above it the table lives in the workspace. */
void wt_smooth_tracks_limits(int32_t* lds_trajectories);
size_t wt_smooth_tracks_workspace(int32_t n_jobs, int32_t n_streams, int64_t n_rows, int64_t n_traj_total, int64_t max_traj);
int wt_smooth_tracks_dev(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                         int32_t r_sets, int64_t n_rows, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                         const double* x, const double* y, const double* w, const double* h, const int32_t* category, const int32_t* local,
                         const int64_t* traj_offsets, int64_t n_traj_total, int64_t max_traj,
                         int32_t n_jobs, const int32_t* job_result, const int32_t* job_window, const double* job_weights,
                         int32_t n_weights, int32_t n_classes, const int64_t* job_row_offsets, int64_t n_out_rows,
                         double* out_bbox, int32_t* out_pairs,
                         int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream);
int wt_smooth_tracks_host(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                          int32_t r_sets, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                          const double* x, const double* y, const double* w, const double* h, const int32_t* category, const int32_t* local,
                          const int32_t* n_traj, int32_t n_jobs, const int32_t* job_result, const int32_t* job_window,
                          const double* job_weights, int32_t n_weights, int32_t n_classes,
                          double* out_bbox, int32_t* out_pairs);

/* =================================================================================================
 * Track deduplication (track-level non-maximum suppression; the definition is DESIGN.md section 23)
 * ================================================================================================= */

/* Suppresses duplicate trajectories of R >= 1 tracking results under J jobs: job j names a result, job_result[j], and its
 * parameters.  Results, frame slots, streams, trajectories, local indices and a trajectory's class (the category of its first
 * observation) are those of the track refinement above; as in stitching the local indices number the trajectories of a
 * (result, stream) by first appearance.  For a trajectory t: n_t = its rows, c_t = its class, s_t = its score sum (0.0, then
 * every row's score added one by one in slot order, float64).  t is stronger than u when n_t > n_u, or n_t == n_u and s_t > s_u,
 * or both are equal and t < u by local index; scores must be finite, so the order is strict and total.
 * m(t, u) = the frame slots in which both have a row and a = iou_dd([x, y, x + w, y + h]_t, [..]_u) satisfies a >= dup_iou[c]
 * and a > 0 (a NaN never does).  t and u are duplicates when c_t == c_u == c, min_frames[c] > 0, m(t, u) >= min_frames[c] and
 * (double)m(t, u) >= dup_frac[c] * (double)min(n_t, n_u) (one multiplication, rounded in float64).
 * The trajectories of a (result, stream) are walked from strongest to weakest; one is suppressed when some stronger trajectory
 * that was itself kept is its duplicate (greedy non-maximum suppression: a suppressed trajectory suppresses nothing).  All rows
 * of a suppressed trajectory are removed; nothing else changes.
 *
 * Jobs: job_result (J) int32, job_min_frames (J, n_classes) int32 >= 0 (0: the class is untouched), job_dup_iou (J, n_classes)
 * float64 not NaN, job_dup_frac (J, n_classes) float64 in [0, 1].
 * Outputs, sized up front: out_keep, out_by, out_match (J, n_traj_total) int32, indexed like traj_offsets - 1 kept / 0
 * suppressed, the local index of the strongest kept duplicate or -1, m with it or 0; out_row_keep (J, n_rows) int32 = per row
 * of the job's result 1 or 0; out_dropped (J, n_streams) int64 = the trajectories suppressed.  Entries of results the job does
 * not name are -1.  A job whose min_frames is all 0 keeps everything.
 *
 * wt_dedup_tracks_dev: device pointers, stream-ordered, no allocation, no synchronisation; it reports in status_dev (device
 * int32) 0 or WT_ERR_CAPACITY (counts, indices or offsets that do not fit the rows).  A workspace smaller than
 * wt_dedup_tracks_workspace() says is WT_ERR_CAPACITY; that size depends on its five arguments only, never on how many
 * duplicates the data holds.  The device form does not check the layout; the host form does (WT_ERR_INVALID names the result
 * and the row or frame slot, or the job and class; a score that is not finite is refused), stages and launches; it takes n_traj
 * (R, n_streams) int32 where the device form takes the running sum traj_offsets, n_traj_total and max_traj.
 * wt_dedup_tracks_limits: the trajectory count of one (result, stream) up to which the tables of the matching stay in LDS;
 * above it they live in the workspace.
 * wt_dedup_tracks_rounds: after a wt_dedup_tracks_dev call on `workspace` has finished, the sweeps over the slots that the
 * matching of each (job, stream) took - 1 + the longest chain of duplicates it had to resolve - into out_rounds (J, n_streams)
 * int32, a host pointer.  It synchronises; it is for measurements. */
void wt_dedup_tracks_limits(int32_t* lds_trajectories);
size_t wt_dedup_tracks_workspace(int32_t n_jobs, int32_t n_streams, int64_t n_rows, int64_t n_traj_total, int64_t max_traj);
int wt_dedup_tracks_rounds(const void* workspace, int32_t n_jobs, int32_t n_streams, int32_t* out_rounds);
int wt_dedup_tracks_dev(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                        int32_t r_sets, int64_t n_rows, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                        const double* x, const double* y, const double* w, const double* h, const double* score,
                        const int32_t* category, const int32_t* local,
                        const int64_t* traj_offsets, int64_t n_traj_total, int64_t max_traj,
                        int32_t n_jobs, const int32_t* job_result, const int32_t* job_min_frames,
                        const double* job_dup_iou, const double* job_dup_frac, int32_t n_classes,
                        int32_t* out_keep, int32_t* out_by, int32_t* out_match, int32_t* out_row_keep, int64_t* out_dropped,
                        int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream);
int wt_dedup_tracks_host(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                         int32_t r_sets, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                         const double* x, const double* y, const double* w, const double* h, const double* score,
                         const int32_t* category, const int32_t* local,
                         const int32_t* n_traj, int32_t n_jobs, const int32_t* job_result, const int32_t* job_min_frames,
                         const double* job_dup_iou, const double* job_dup_frac, int32_t n_classes,
                         int32_t* out_keep, int32_t* out_by, int32_t* out_match, int32_t* out_row_keep, int64_t* out_dropped);

/* =================================================================================================
 * Cross-class track suppression (duplicates across classes; the definition is DESIGN.md section 26)
 * ================================================================================================= */

/* Suppresses trajectories that are the same object as a stronger one of ANOTHER class (a pedestrian track on the rider of a
 * tracked cyclist) under J jobs.  Results, slots, streams, trajectories, local indices, c_t, n_t and s_t are those of the track
 * deduplication above.  A job carries pair_frames[a][b] int32 >= 0 (0: the pair of classes a + 1 and b + 1 is off),
 * pair_overlap[a][b] float64 not NaN, pair_frac[a][b] float64 in [0, 1] - three (n_classes, n_classes) tables that must be
 * symmetric, the doubles bit for bit; the diagonal means pairs inside a class - class_prio[c] int32 and measure (0 = IoU,
 * 1 = IoMin); n_classes <= 16.  A trajectory whose class is outside 1..n_classes takes part in no pair.
 * Measure of two boxes [x1, y1, x2, y2], with w, h, wh, area_a, area_b as iou_dd computes them: IoU = iou_dd; IoMin = wh / lo,
 * lo the smaller area, and only when area_a > 0, area_b > 0 and both are finite (otherwise the slot does not match).  A slot
 * matches when v >= pair_overlap[c_t][c_u] and v > 0; m(t, u) counts the matching slots.
 * t is stronger than u by: higher class_prio[c], then more rows, then higher score sum, then lower local index (strict, total;
 * scores must be finite).  t and u are the same object when pair_frames[c_t][c_u] > 0, m(t, u) >= pair_frames[c_t][c_u] and
 * (double)m(t, u) >= pair_frac[c_t][c_u] * (double)n_weak, n_weak the rows of the WEAKER of the two (one multiplication, rounded
 * in float64).  Greedy suppression and the outputs are those of the deduplication: out_keep, out_by, out_match (J, n_traj_total),
 * out_row_keep (J, n_rows), out_dropped (J, n_streams); entries of results the job does not name are -1.  A job whose
 * pair_frames is all 0 keeps everything.
 *
 * The five entry points are the twins of wt_dedup_tracks_*: the device form takes device pointers, is stream-ordered, never
 * allocates or waits, reports 0 or WT_ERR_CAPACITY in status_dev, answers a workspace smaller than
 * wt_xclass_tracks_workspace() with WT_ERR_CAPACITY before any launch and does not check the layout (it reads the tables at
 * (lower class, higher class) only); the host form checks (WT_ERR_INVALID names the result and the row or frame slot, or the
 * job and the pair), stages and launches. */
void wt_xclass_tracks_limits(int32_t* lds_trajectories);
size_t wt_xclass_tracks_workspace(int32_t n_jobs, int32_t n_streams, int64_t n_rows, int64_t n_traj_total, int64_t max_traj);
int wt_xclass_tracks_rounds(const void* workspace, int32_t n_jobs, int32_t n_streams, int32_t* out_rounds);
int wt_xclass_tracks_dev(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                         int32_t r_sets, int64_t n_rows, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                         const double* x, const double* y, const double* w, const double* h, const double* score,
                         const int32_t* category, const int32_t* local,
                         const int64_t* traj_offsets, int64_t n_traj_total, int64_t max_traj,
                         int32_t n_jobs, const int32_t* job_result, const int32_t* job_pair_frames,
                         const double* job_pair_overlap, const double* job_pair_frac, const int32_t* job_class_prio,
                         const int32_t* job_measure, int32_t n_classes,
                         int32_t* out_keep, int32_t* out_by, int32_t* out_match, int32_t* out_row_keep, int64_t* out_dropped,
                         int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream);
int wt_xclass_tracks_host(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                          int32_t r_sets, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                          const double* x, const double* y, const double* w, const double* h, const double* score,
                          const int32_t* category, const int32_t* local,
                          const int32_t* n_traj, int32_t n_jobs, const int32_t* job_result, const int32_t* job_pair_frames,
                          const double* job_pair_overlap, const double* job_pair_frac, const int32_t* job_class_prio,
                          const int32_t* job_measure, int32_t n_classes,
                          int32_t* out_keep, int32_t* out_by, int32_t* out_match, int32_t* out_row_keep, int64_t* out_dropped);

/* =================================================================================================
 * Cross-class track linking (class flicker: tracklets linked across classes and relabelled; the definition is DESIGN.md section 31)
 * ================================================================================================= */

/* Links the trajectories of R >= 1 tracking results across gaps AND classes under J jobs, and gives every chain one class.
 * Results, slots, streams, trajectories, local indices (by first appearance), a trajectory's class, the affinity a of a tail and a
 * head, and the walk of the candidates in the strict order (-a, n, i, j) are those of the track stitching above.  What differs is
 * rule 1: tail i of class ci and head j != i of the same stream and class cj are a candidate when n lies in
 * 1..pair_max_link[ci][cj], a >= pair_link_iou[ci][cj] and a > 0.  A job carries pair_max_link int32 >= 0 (0: the pair is off)
 * and pair_link_iou float64 not NaN - two (n_classes, n_classes) tables that must be symmetric, the doubles bit for bit; the
 * diagonal means pairs inside a class - class_prio[c] int32 and motion (0 = hold, 1 = linear); n_classes <= 16.
 * A chain is a root and everything linked behind it.  Its class is the class c that maximises (rows of the chain's trajectories
 * whose class is c, class_prio[c], 1 if c is the root's class else 0, -c) among the classes with at least one row: integers only.
 *
 * Outputs, sized up front: out_pred, out_root (J, n_traj_total) int32 and out_affinity (J, n_traj_total) float64 as in the
 * stitching; out_cls (J, n_traj_total) int32 = the chain's class at every member; out_row_root, out_row_category (J, n_rows)
 * int32 = per row of the job's result the root's local index and the chain's class; out_links, out_relabelled (J, n_streams)
 * int64 = the links made and the rows whose category changed.  Entries of results the job does not name are -1 (-1.0).
 *
 * The entry points are the twins of wt_stitch_tracks_*: the device form takes device pointers, is stream-ordered, never allocates
 * or waits, reports 0 or WT_ERR_CAPACITY in status_dev, answers a workspace smaller than wt_xlink_tracks_workspace() with
 * WT_ERR_CAPACITY and more than 16 classes with WT_ERR_INVALID before any launch, and does not check the layout; the host form
 * checks (WT_ERR_INVALID names the result and the row or frame slot, or the job and the pair), stages and launches.
 * wt_xlink_tracks_limits: the trajectory count of one (result, stream) up to which the tables of the matching stay in LDS.
 * wt_xlink_tracks_rounds: after a finished call on `workspace`, the rounds that accepted a link, (J, n_streams); it synchronises. */
void wt_xlink_tracks_limits(int32_t* lds_trajectories);
size_t wt_xlink_tracks_workspace(int32_t n_jobs, int32_t n_streams, int64_t n_rows, int64_t n_traj_total, int64_t max_traj);
int wt_xlink_tracks_rounds(const void* workspace, int32_t n_jobs, int32_t n_streams, int32_t* out_rounds);
int wt_xlink_tracks_dev(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                        int32_t r_sets, int64_t n_rows, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                        const double* x, const double* y, const double* w, const double* h, const int32_t* category, const int32_t* local,
                        const int64_t* traj_offsets, int64_t n_traj_total, int64_t max_traj,
                        int32_t n_jobs, const int32_t* job_result, const int32_t* job_pair_max_link, const double* job_pair_link_iou,
                        const int32_t* job_class_prio, const int32_t* job_motion, int32_t n_classes,
                        int32_t* out_pred, int32_t* out_root, double* out_affinity, int32_t* out_cls, int32_t* out_row_root,
                        int32_t* out_row_category, int64_t* out_links, int64_t* out_relabelled,
                        int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream);
int wt_xlink_tracks_host(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets,
                         int32_t r_sets, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                         const double* x, const double* y, const double* w, const double* h, const int32_t* category, const int32_t* local,
                         const int32_t* n_traj, int32_t n_jobs, const int32_t* job_result, const int32_t* job_pair_max_link,
                         const double* job_pair_link_iou, const int32_t* job_class_prio, const int32_t* job_motion, int32_t n_classes,
                         int32_t* out_pred, int32_t* out_root, double* out_affinity, int32_t* out_cls, int32_t* out_row_root,
                         int32_t* out_row_category, int64_t* out_links, int64_t* out_relabelled);

/* =================================================================================================
 * Detection evaluation (VOC-style AP / AR per class, IoU threshold and box-size bucket; the definition is DESIGN.md section 16)
 * ================================================================================================= */

/* Scores K >= 1 detection results against one ground truth, as detnet/data/metric.py does on one host thread (match_class,
 * _curves, voc_ap in the non-07 form): every detection takes the ground-truth box of highest IoU (the first one, numpy argmax)
 * and is a true positive at threshold t when that IoU exceeds t and it is the most confident detection claiming that box.
 * Equal confidences keep the input order: image order, then row order inside the image.
 *
 * Ground truth: SoA rows in image order - x1, y1, x2, y2 float64 normalised, label int32 in 1..n_classes - with the CSR offsets
 * image_gt_offsets (n_images + 1) and image_area (n_images) float64 = width * height in pixels.
 * Results: the K sets concatenated; set k owns rows set_row_offsets[k] .. set_row_offsets[k + 1], in image order (file order
 * inside an image), image_det_offsets[k * (n_images + 1) + i] = offsets of image i inside the set.  conf, cx, cy, w, h float64
 * normalised, category int32 in 1..n_classes.  A row takes part when conf > min_conf[k] (min_conf: K values, host pointer).
 * thr: (n_classes, n_thr) IoU thresholds, host pointer; both host arrays are read before the call returns: thr travels as a kernel
 * argument, min_conf in one hipMemcpyAsync of K doubles from the caller's (pageable) memory, which the runtime stages before it
 * returns and which keeps the device form out of a hipGraph capture.  n_classes <= 16, n_thr <= 8; no limit on the rows of one image; K x n_images x n_classes
 * below 2^26 and K x n_classes x n_thr below 2^21 (one workgroup each; more is WT_ERR_CAPACITY).
 * Outputs: ap, ar float64 and npos, tp, fp int64, each (K, n_classes, n_thr, 4): buckets '' (all sizes), S, M, L of the box area
 *          in pixels (< 32^2, < 96^2, the rest); ar is NaN without rows;
 *          per row, each may be NULL: tp_flag (n_det, n_thr) uint8 1 = TP, 0 = FP, 2 = took no part; match_gt (n_det) the
 *          ground-truth row of highest IoU, -1 when there is none; order (n_det) the row indices sorted by (set, class,
 *          descending confidence), rows that took no part last; class_offsets (K, n_classes + 1) positions in `order`;
 *          ctp, cfp (n_det, n_thr) int64: cumulative TP / FP of the all-sizes bucket at every position of `order` (together).
 * The device form takes device pointers (except min_conf and thr), never synchronises or allocates and reports 0 or a WT_ERR_*
 * in status_dev (device int32); it does not check the layout, the host form does (WT_ERR_INVALID names the set / image / row). */
size_t wt_det_eval_workspace(int32_t k_sets, int64_t n_images, int32_t n_classes, int32_t n_thr, int64_t n_gt, int64_t n_det);
int wt_det_eval_dev(int64_t n_gt, const double* gx1, const double* gy1, const double* gx2, const double* gy2, const int32_t* g_label,
                    int64_t n_images, const int64_t* image_gt_offsets, const double* image_area,
                    int32_t k_sets, int64_t n_det, const int64_t* set_row_offsets, const int64_t* image_det_offsets,
                    const double* conf, const double* cx, const double* cy, const double* w, const double* h, const int32_t* category,
                    const double* min_conf, int32_t n_classes, int32_t n_thr, const double* thr,
                    double* ap, double* ar, int64_t* npos, int64_t* tp, int64_t* fp,
                    uint8_t* tp_flag, int64_t* match_gt, int64_t* order, int64_t* class_offsets, int64_t* ctp, int64_t* cfp,
                    int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream);
int wt_det_eval_host(int64_t n_gt, const double* gx1, const double* gy1, const double* gx2, const double* gy2, const int32_t* g_label,
                     int64_t n_images, const int64_t* image_gt_offsets, const double* image_area,
                     int32_t k_sets, const int64_t* set_row_offsets, const int64_t* image_det_offsets,
                     const double* conf, const double* cx, const double* cy, const double* w, const double* h, const int32_t* category,
                     const double* min_conf, int32_t n_classes, int32_t n_thr, const double* thr,
                     double* ap, double* ar, int64_t* npos, int64_t* tp, int64_t* fp,
                     uint8_t* tp_flag, int64_t* match_gt, int64_t* order, int64_t* class_offsets, int64_t* ctp, int64_t* cfp);

/* =================================================================================================
 * COCO detection evaluation (AP@[.5:.95], AP50, AP75, by area, AR@1/10/100; the definition is DESIGN.md section 28)
 * ================================================================================================= */

/* Scores K >= 1 detection results against one ground truth with the COCO rule: per (image, category) the detections by
 * descending score (equal scores in input order), the first max_dets[last] of them; per area range and IoU threshold a greedy
 * one-to-one match to the best ground-truth box that is still free (ties to the later box), not-ignored boxes before ignored
 * ones, crowd boxes never used up; precision read at n_rec recall thresholds from the curve made non-increasing from the right.
 *
 * Ground truth: SoA rows in image order - gx, gy, gw, gh pixel [x, y, w, h] and g_area float64, g_cat int32 category index in
 * 0..n_cats-1, g_crowd uint8 - with the CSR offsets image_gt_offsets (n_images + 1).
 * Results: the K sets concatenated; set k owns rows set_row_offsets[k] .. set_row_offsets[k + 1], in image order (input order
 * inside an image), image_det_offsets[k * (n_images + 1) + i] = offsets of image i inside the set.  score, x, y, w, h float64
 * pixels, category int32 index in 0..n_cats-1.  image_mask: NULL, or (K, n_images) uint8 - 0 takes the image out of result k
 * (its rows and its ground truth).
 * Host arrays, read before the call returns (they travel as kernel arguments, so the device form can be captured in a graph):
 * thr (n_thr <= 16) IoU thresholds, rec (n_rec <= 128) ascending recall thresholds, area_rng (n_area <= 4, 2) inclusive
 * [lo, hi] pairs with n_area * n_thr <= 64, max_dets (n_maxdet <= 4) ascending, at most 128.  No limit on the rows of one
 * image or problem; K x n_images x n_cats below 2^26 and K x n_cats x n_area x n_maxdet x n_thr below 2^24 (one workgroup
 * each; more is WT_ERR_CAPACITY).
 * Outputs: precision (K, n_thr, n_rec, n_cats, n_area, n_maxdet) and recall (K, n_thr, n_cats, n_area, n_maxdet) float64, -1
 *          where the category has no not-ignored ground truth; npig (K, n_cats, n_area) int64, that count;
 *          per row, each may be NULL: rank (n_det) int32 position in its problem, -1 = beyond max_dets[last] or took no part;
 *          match_gt (n_det, n_area, n_thr) int64 ground-truth row, -1 none; ignore (n_det, n_area, n_thr) uint8 (together).
 * The device form takes device pointers (except the four host arrays), never synchronises or allocates and reports 0 or a
 * WT_ERR_* in status_dev (device int32); it does not check the layout or the numbers and only stays in bounds on non-finite
 * rows; the host form checks both (WT_ERR_INVALID names the set / image / row).  Every refusal comes before any launch. */
size_t wt_det_coco_workspace(int32_t k_sets, int64_t n_images, int32_t n_cats, int32_t n_thr, int32_t n_rec, int32_t n_area, int32_t n_maxdet,
                             int64_t n_gt, int64_t n_det);
int wt_det_coco_dev(int64_t n_gt, const double* gx, const double* gy, const double* gw, const double* gh, const double* g_area,
                    const int32_t* g_cat, const uint8_t* g_crowd, int64_t n_images, const int64_t* image_gt_offsets,
                    int32_t k_sets, int64_t n_det, const int64_t* set_row_offsets, const int64_t* image_det_offsets,
                    const double* score, const double* x, const double* y, const double* w, const double* h, const int32_t* category,
                    const uint8_t* image_mask, int32_t n_cats, int32_t n_thr, const double* thr, int32_t n_rec, const double* rec,
                    int32_t n_area, const double* area_rng, int32_t n_maxdet, const int32_t* max_dets,
                    double* precision, double* recall, int64_t* npig, int32_t* rank, int64_t* match_gt, uint8_t* ignore,
                    int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream);
int wt_det_coco_host(int64_t n_gt, const double* gx, const double* gy, const double* gw, const double* gh, const double* g_area,
                     const int32_t* g_cat, const uint8_t* g_crowd, int64_t n_images, const int64_t* image_gt_offsets,
                     int32_t k_sets, const int64_t* set_row_offsets, const int64_t* image_det_offsets,
                     const double* score, const double* x, const double* y, const double* w, const double* h, const int32_t* category,
                     const uint8_t* image_mask, int32_t n_cats, int32_t n_thr, const double* thr, int32_t n_rec, const double* rec,
                     int32_t n_area, const double* area_rng, int32_t n_maxdet, const int32_t* max_dets,
                     double* precision, double* recall, int64_t* npig, int32_t* rank, int64_t* match_gt, uint8_t* ignore);

/* =================================================================================================
 * Track layouts (the two steps between the tracker, the post-passes and the metrics; the definitions are DESIGN.md section 29)
 * ================================================================================================= */

/* wt_tracks_layout_*: R >= 1 tracker outputs, each in buffers of its own, -> the shared layout of the post-passes ("Track
 * refinement" above: "Results: the R sets concatenated, SoA ...") without the rows leaving the device.
 *
 * Input of the device form: in_tables, device int64 (R, 7) - per result the addresses of out_frame int64 (the global frame slot),
 * out_category int32, out_bbox (n, 4) float64, out_score float64, out_object_id int64 and of the row count, a device int64, as
 * wt_track_streams_dev / wt_track_streams_byte_dev leave them, and the row capacity of those buffers.  A negative count is the
 * tracker's error status and becomes the call's status; a count above its capacity, or more rows in all than out_cap, is
 * WT_ERR_CAPACITY.  The rows of a result must ascend by frame slot (the tracker's do); the kernels check that they do, that the
 * slots lie in 0..n_frames-1 and the categories in 1..n_classes, and that stream_frame_offsets (n_streams + 1, device) cover
 * the slots: WT_ERR_INVALID otherwise.  On any status the outputs are unspecified, and nothing is written out of bounds.  The
 * same trajectory twice in one slot is not checked, as in the other device forms.
 * Output, every array sized by the caller: x, y, w, h, score float64 and category int32 (out_cap), bit-copies of the input;
 * local int32 (out_cap) = the row's trajectory - the rows of one (result, stream) with one object id - numbered from 0 by first
 * appearance in row order; set_row_offsets (R + 1); frame_row_offsets (R, n_frames + 1); n_traj (R, n_streams) int32 and its
 * running sum traj_offsets (R * n_streams + 1) int64; totals (3) int64 = the rows of all results, n_traj_total, max_traj;
 * traj_object_id (out_cap) int64, indexed like traj_offsets = the object id of the trajectory's first row.
 * Integers and bit-copies only: the answer is exact and the same for every launch.
 *
 * One workgroup per (result, stream) keeps an open-addressing table of the stream's ids: in LDS (lds_slots slots) while the
 * stream has at most lds_rows rows, in the workspace (2 x its rows) above; wt_tracks_layout_limits reports both and scan_rows,
 * the rows a workgroup scans per step.  wt_tracks_layout_probe is the first slot the table tries for `id` at `capacity` slots
 * (-1 for a capacity below 1), the later ones following linearly: host code, for tests that need ids which collide.
 * The device form takes device pointers, is stream-ordered, never allocates or synchronises, and reports 0 or a WT_ERR_* in
 * status_dev (device int32).  Bad arguments are WT_ERR_INVALID, a workspace below wt_tracks_layout_workspace() bytes, more than
 * 65535 results or 2^31 (result, stream) pairs WT_ERR_CAPACITY, all before any launch; the sizer returns 0 for a bad shape.
 * The host form takes the R results back to back - in_row_offsets (R + 1), then the five columns - checks them (WT_ERR_INVALID
 * names the result and the row), stages, calls the device form and copies back; its outputs hold in_row_offsets[R] rows. */
void wt_tracks_layout_limits(int32_t* lds_rows, int32_t* lds_slots, int32_t* scan_rows);
int32_t wt_tracks_layout_probe(int64_t id, int32_t capacity);
size_t wt_tracks_layout_workspace(int32_t r_sets, int32_t n_streams, int64_t out_cap);
int wt_tracks_layout_dev(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets, int32_t r_sets, const int64_t* in_tables,
                         int32_t n_classes, int64_t out_cap,
                         double* x, double* y, double* w, double* h, double* score, int32_t* category, int32_t* local,
                         int64_t* set_row_offsets, int64_t* frame_row_offsets, int32_t* n_traj, int64_t* traj_offsets, int64_t* totals,
                         int64_t* traj_object_id, int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream);
int wt_tracks_layout_host(int64_t n_frames, int32_t n_streams, const int64_t* stream_frame_offsets, int32_t r_sets, const int64_t* in_row_offsets,
                          const int64_t* in_frame, const int32_t* in_category, const double* in_bbox, const double* in_score, const int64_t* in_object_id,
                          int32_t n_classes,
                          double* x, double* y, double* w, double* h, double* score, int32_t* category, int32_t* local,
                          int64_t* set_row_offsets, int64_t* frame_row_offsets, int32_t* n_traj, int64_t* traj_offsets, int64_t* totals,
                          int64_t* traj_object_id);

/* wt_tracks_to_eval_*: K >= 1 results in the shared layout -> the rows in the order wt_mot_*_dev take them ("MOT evaluation"
 * above: "Results: the K sets concatenated ...").
 *
 * Input: set_row_offsets (K + 1, the first 0), frame_row_offsets (K, n_frames + 1) - rows behind a set's last offset take no
 * part -, category and local int32, and the boxes x, y, w, h float64 with row i at [i * box_stride]: 1 for the columns
 * wt_tracks_layout_* writes, 4 for out_bbox, out_bbox + 1, ... of wt_refine_tracks_emit_dev, whose job_row_offsets and
 * out_frame_row_offsets are the two offset arrays.  slot_map (n_frames) int64: per frame slot the ground truth's frame slot, or
 * -1 where the ground truth has no such frame or stream; no ground-truth slot is named twice.
 * Output, per result in its input rows' place: first the rows on a known slot with a category in 1..n_classes, by ground-truth
 * slot and in input order inside a slot, then the others in input order.  out_x, out_y, out_w, out_h float64 (bit-copies),
 * out_category, out_h_id int32 (= local: equal inside a (result, stream) <=> one trajectory, all wt_mot_eval_* asks of it),
 * out_order int64 = the output row's input row inside its result (n_rows each); out_set_row_offsets (K + 1);
 * frame_hyp_offsets (K, n_gt_frames + 1); max_frame_boxes, one int64 = the most rows of one class on one known slot.
 * The device form takes device pointers and n_rows = an upper bound of set_row_offsets[K] that the outputs hold, is
 * stream-ordered, never allocates or synchronises, and reports 0 or WT_ERR_INVALID (offsets that do not fit the rows, a map
 * entry outside -1..n_gt_frames-1 or named twice, a negative local index) in status_dev; the outputs are then unspecified and
 * nothing is written out of bounds.  Bad arguments are WT_ERR_INVALID and a workspace below wt_tracks_to_eval_workspace() bytes
 * WT_ERR_CAPACITY before any launch.  The host form checks the layout and the map (WT_ERR_INVALID names the result or the
 * slots), stages, calls the device form and copies back. */
size_t wt_tracks_to_eval_workspace(int32_t k_sets, int64_t n_rows);
int wt_tracks_to_eval_dev(int64_t n_frames, int32_t k_sets, int64_t n_rows, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                          const double* x, const double* y, const double* w, const double* h, int64_t box_stride,
                          const int32_t* category, const int32_t* local, const int64_t* slot_map, int64_t n_gt_frames, int32_t n_classes,
                          double* out_x, double* out_y, double* out_w, double* out_h, int32_t* out_category, int32_t* out_h_id,
                          int64_t* out_set_row_offsets, int64_t* frame_hyp_offsets, int64_t* out_order, int64_t* max_frame_boxes,
                          int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream);
int wt_tracks_to_eval_host(int64_t n_frames, int32_t k_sets, const int64_t* set_row_offsets, const int64_t* frame_row_offsets,
                           const double* x, const double* y, const double* w, const double* h, int64_t box_stride,
                           const int32_t* category, const int32_t* local, const int64_t* slot_map, int64_t n_gt_frames, int32_t n_classes,
                           double* out_x, double* out_y, double* out_w, double* out_h, int32_t* out_category, int32_t* out_h_id,
                           int64_t* out_set_row_offsets, int64_t* frame_hyp_offsets, int64_t* out_order, int64_t* max_frame_boxes);

/* --- Waymo Open Dataset protobuf emit (csrc/waymo_proto.hip; host code) -----------------------------------
 * metrics.Objects - and with submission != 0 the Submission envelope around it - written straight from columns: replaces
 * the per-object message building of /root/reference/coco_to_waymo.py:16-82 (create_pd_object / create_pb_submission) and
 * generate_prediction_for_metrics.py:43-80 (metrics_mode = 1: explicit zero z / height / heading, num_lidar_points_in_box =
 * 100).  context / id: UTF-8 blob + n+1 offsets; has_id NULL = every row has an id when id_offsets is given; score NULL = not
 * set (ground truth); det_level / trk_level NULL or 0 = not set; authors = n_authors NUL-terminated strings back to back.
 * Field numbers are recalled from the public waymo-open-dataset .proto files (the package is not in the image). */
int wt_waymo_objects_write(const char* path, int64_t n, const char* context_blob, const int64_t* context_offsets,
                           const int64_t* frame_timestamp_micros, const int32_t* camera_name, const double* bbox_xywh,
                           const double* score, const int32_t* label_type, const char* id_blob, const int64_t* id_offsets,
                           const uint8_t* has_id, const int32_t* det_level, const int32_t* trk_level, int metrics_mode,
                           int submission, int task, const char* account_name, const char* unique_method_name,
                           const char* authors, int n_authors, const char* affiliation, const char* description,
                           int sensor_type, int64_t* bytes_written);

#ifdef __cplusplus
}
#endif
#endif
