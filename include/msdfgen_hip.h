/*
 * msdfgen_hip.h -- C ABI of the MI355X-native MSDF hot path (libmsdfgen_hip.so).
 *
 * Drop-in boundary for the per-texel signed-distance path of Chlumsky/msdfgen v1.13.0.  Each entry point names the
 * reference interface it replaces (file:line relative to the reference tree).  Plain pointers and sizes only.
 *
 * Shape encoding (the reference's `const Shape &`, core/Shape.h:15-58, flattened once by the caller/binding):
 *   contour_offsets int32[n_contours+1]  CSR offsets into the edge arrays; edges of a contour in Shape order
 *   points          double[n_edges*8]    p0x,p0y,p1x,p1y,p2x,p2y,p3x,p3y (unused slots ignored)
 *   types           uint8[n_edges]       1 linear, 2 quadratic, 3 cubic       (EDGE_TYPE, core/edge-segments.h:62,91,122)
 *   colors          uint8[n_edges]       EdgeColor bitmask R=1 G=2 B=4        (core/EdgeColor.h:9-18)
 *
 * Transformation (the reference's `const SDFTransformation &`, core/SDFTransformation.h:13-24):
 *   xf[6] = { Projection.scale.x, .scale.y, .translate.x, .translate.y,      (core/Projection.h:31-33)
 *             DistanceMapping.scale, DistanceMapping.translate }             (core/DistanceMapping.h:28-30)
 *   i.e. texel centre (x+.5, y+.5) -> shape point  coord/scale - translate  (core/Projection.cpp:14-16)
 *        distance d -> float(mapScale*(d+mapTranslate))                      (core/DistanceMapping.cpp:15-17)
 *
 * Output bitmap (the reference's `const BitmapSection<float, N> &`, core/BitmapRef.hpp:74-111):
 *   pixels, width, height, row_stride (in floats, may be negative), channel-interleaved.
 *   `flip` != 0 when shape.getYAxisOrientation() != bitmap.yOrientation: rows are then written in reverse
 *   (BitmapSection::reorient, core/BitmapRef.hpp:103-109).
 *
 * All functions return MSDFHIP_OK (0) or a negative MSDFHIP_ERR_* code; msdfhip_last_error() gives the text.
 * There is NO CPU fallback: without a usable gfx950 device every compute entry point fails with MSDFHIP_ERR_NO_DEVICE.
 * Thread safety: all entry points may be called concurrently from many host threads (the reference's generate* functions
 * are re-entrant); host-pointer calls use a per-thread stream and staging buffers.
 */
#ifndef MSDFGEN_HIP_H
#define MSDFGEN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSDFHIP_ABI_VERSION 5

/* mode: which generator (msdfgen.h:46-56) */
#define MSDFHIP_MODE_SDF   1 /* generateSDF   msdfgen.h:47  (TrueDistanceSelector)          1 channel  */
#define MSDFHIP_MODE_PSDF  2 /* generatePSDF  msdfgen.h:49  (PerpendicularDistanceSelector) 1 channel  */
#define MSDFHIP_MODE_MSDF  3 /* generateMSDF  msdfgen.h:51  (MultiDistanceSelector)         3 channels */
#define MSDFHIP_MODE_MTSDF 4 /* generateMTSDF msdfgen.h:53  (MultiAndTrueDistanceSelector)  4 channels */

/* ErrorCorrectionConfig::Mode, core/generator-config.h:20-29 */
#define MSDFHIP_EC_DISABLED       0
#define MSDFHIP_EC_INDISCRIMINATE 1
#define MSDFHIP_EC_EDGE_PRIORITY  2
#define MSDFHIP_EC_EDGE_ONLY      3
/* ErrorCorrectionConfig::DistanceCheckMode, core/generator-config.h:31-38 */
#define MSDFHIP_DO_NOT_CHECK_DISTANCE  0
#define MSDFHIP_CHECK_DISTANCE_AT_EDGE 1
#define MSDFHIP_ALWAYS_CHECK_DISTANCE  2

#define MSDFHIP_OK                  0
#define MSDFHIP_ERR_NO_DEVICE      -1 /* no HIP device / not gfx950 / runtime error at init */
#define MSDFHIP_ERR_INVALID        -2 /* bad argument */
#define MSDFHIP_ERR_HIP            -3 /* a HIP call failed; see msdfhip_last_error() */
#define MSDFHIP_ERR_TOO_COMPLEX    -4 /* (round 3: no longer returned for large shapes -- they take list-free kernels; kept for the error-correction
                                         kernel's fixed LDS exceeding a device's limit, which no gfx950 input reaches) */
#define MSDFHIP_ERR_NOMEM          -5

/* MSDFGeneratorConfig + ErrorCorrectionConfig (core/generator-config.h:13-64) without the buffer pointer. */
typedef struct MsdfHipConfig {
    int32_t overlap_support;     /* GeneratorConfig::overlapSupport, default 1 */
    int32_t ec_mode;             /* default MSDFHIP_EC_EDGE_PRIORITY */
    int32_t ec_distance_check;   /* default MSDFHIP_CHECK_DISTANCE_AT_EDGE */
    int32_t ec_stage_limit;      /* 0 = full pipeline. 1..4: debug -- stop the stencil pipeline after stage k of
                                    core/msdf-error-correction.cpp:27-46 (1 protectCorners, 2 +protectEdges, 3 +findErrors(sdf),
                                    4 +protectAll+findErrors(sdf,shape)) and do not apply; used by the parity tests */
    double min_deviation_ratio;  /* default 1.11111111111111111 (core/MSDFErrorCorrection.cpp:22) */
    double min_improve_ratio;    /* default 1.11111111111111111 (core/MSDFErrorCorrection.cpp:23) */
    /* Optional scanline pass between the distance field and the error correction, as the reference CLI does in no-Skia builds
     * (main.cpp:1281-1298): distanceSignCorrection (core/rasterization.h:17-19). Default off (the library functions do not do it). */
    int32_t sign_correction;     /* 0 / 1 */
    int32_t fill_rule;           /* FillRule, core/Scanline.h:10-15: 0 NONZERO (default), 1 ODD, 2 POSITIVE, 3 NEGATIVE */
    float sdf_zero_value;        /* default 0.5 */
    int32_t stencil_y_down;      /* 1: the output bitmap's yOrientation is Y_DOWNWARD. Only the row order of the optional stencil
                                    (ErrorCorrectionConfig::buffer) depends on it: the reference creates the stencil section with the
                                    default orientation (core/msdf-error-correction.cpp:19) and re-orients it against the bitmap
                                    (core/MSDFErrorCorrection.cpp:122,192,415), so its memory row r is always the r-th row counted
                                    upwards -- the bitmap's memory row height-1-r when the bitmap is Y_DOWNWARD. Default 0. */
} MsdfHipConfig;

/* Per-glyph descriptor of a batch (one output tile per glyph). Lives in device memory for the *_device entry points. */
typedef struct MsdfHipGlyph {
    double xf[6];                /* sx, sy, tx, ty, mapScale, mapTranslate */
    int64_t out_offset;          /* index (in floats) of texel (0,0) of memory row 0 of this tile in the output buffer */
    int32_t row_stride;          /* floats between consecutive memory rows of the tile (BitmapSection::rowStride) */
    int32_t flip;                /* 1: shape Y orientation != bitmap orientation */
} MsdfHipGlyph;

/* Fills *cfg with the reference's defaults (MSDFGeneratorConfig(), core/generator-config.h:46,53,62). */
void msdfhip_default_config(MsdfHipConfig *cfg);

int msdfhip_abi_version(void);
/* Makes HIP device `device` the process default (checks that it is gfx950): the device of the single-shape calls and of batches
 * created without an explicit device. Batches remember their device; every call on a batch binds the calling thread to it, so one
 * process can drive all GPUs of a node (msdfhip_batch_create_on, msdfhip_generate_sharded below). */
int msdfhip_init(int device);
int msdfhip_device_count(int *count);
/* Text of the last error on the calling thread ("" if none). */
const char *msdfhip_last_error(void);
/* name buffer receives e.g. "gfx950:sramecc+:xnack-"; cus/lds_bytes may be NULL. */
int msdfhip_device_info(char *name, size_t name_len, int *cus, int *lds_bytes);

/* ------------------------------------------------------------------------------------------------------------------
 * Single-shape, host-pointer calls: the literal replacements of the reference's functions.
 * ------------------------------------------------------------------------------------------------------------------ */

/* generateSDF / generatePSDF / generateMSDF / generateMTSDF(output, shape, transformation, config)
 *   replaces core/msdfgen.cpp:78-106 (declared msdfgen.h:46-53); the Projection+Range overloads (msdfgen.h:59-63) and the legacy
 *   Range/scale/translate overloads (msdfgen.h:65-69) forward here after building xf.
 * For modes 3, 4 the error-correction pass (core/msdfgen.cpp:97,105) runs as configured. `stencil` is the optional
 * ErrorCorrectionConfig::buffer (core/generator-config.h:44): NULL, or width*height bytes that receive the final stencil. */
int msdfhip_generate(int mode, float *pixels, int width, int height, int row_stride, int flip,
                     const int32_t *contour_offsets, int n_contours, const double *points, const uint8_t *types, const uint8_t *colors,
                     const double *xf, const MsdfHipConfig *cfg, uint8_t *stencil);

int msdfhip_generate_sdf(float *pixels, int width, int height, int row_stride, int flip,
                         const int32_t *contour_offsets, int n_contours, const double *points, const uint8_t *types, const uint8_t *colors,
                         const double *xf, const MsdfHipConfig *cfg);                      /* msdfgen.h:47 */
int msdfhip_generate_psdf(float *pixels, int width, int height, int row_stride, int flip,
                          const int32_t *contour_offsets, int n_contours, const double *points, const uint8_t *types, const uint8_t *colors,
                          const double *xf, const MsdfHipConfig *cfg);                     /* msdfgen.h:49 */
int msdfhip_generate_msdf(float *pixels, int width, int height, int row_stride, int flip,
                          const int32_t *contour_offsets, int n_contours, const double *points, const uint8_t *types, const uint8_t *colors,
                          const double *xf, const MsdfHipConfig *cfg, uint8_t *stencil);   /* msdfgen.h:51 */
int msdfhip_generate_mtsdf(float *pixels, int width, int height, int row_stride, int flip,
                           const int32_t *contour_offsets, int n_contours, const double *points, const uint8_t *types, const uint8_t *colors,
                           const double *xf, const MsdfHipConfig *cfg, uint8_t *stencil);  /* msdfgen.h:53 */

/* msdfErrorCorrection(sdf, shape, transformation, config) on an existing 3- or 4-channel bitmap, in place.
 *   replaces core/msdf-error-correction.cpp:61-72 (declared core/msdf-error-correction.h:15-18). */
int msdfhip_error_correction(int channels, float *pixels, int width, int height, int row_stride, int flip,
                             const int32_t *contour_offsets, int n_contours, const double *points, const uint8_t *types, const uint8_t *colors,
                             const double *xf, const MsdfHipConfig *cfg, uint8_t *stencil);
/* msdfFastDistanceErrorCorrection (protect_all = 0) / msdfFastEdgeErrorCorrection (protect_all = 1): findErrors(sdf) + apply with no shape.
 *   replaces core/msdf-error-correction.cpp:50-59, 87-113 (declared core/msdf-error-correction.h:21-34). */
int msdfhip_error_correction_shapeless(int channels, float *pixels, int width, int height, int row_stride, const double *xf,
                                       double min_deviation_ratio, int protect_all);

/* The legacy generators: generateSDF_legacy / generatePSDF_legacy / generateMSDF_legacy / generateMTSDF_legacy(output, shape, range, scale, translate
 * [, errorCorrectionConfig]), core/msdfgen.cpp:166-333 (declared msdfgen.h:72-76) -- the minimum over all edges in shape order, no contour combiner.
 * Arguments as msdfhip_generate (xf built from scale, translate and range as there). Of `cfg` only ec_mode, the two ratios, the sign-pass fields
 * (sign_correction, fill_rule, sdf_zero_value) and stencil_y_down are read: the correction of modes 3, 4 always runs without overlap support and with
 * MSDFHIP_DO_NOT_CHECK_DISTANCE, as the reference's does (core/msdfgen.cpp:272-273). With sign_correction this is the reference CLI's -legacy flow
 * (main.cpp:1223-1298). `stencil`: as msdfhip_generate. Set flip = (shape is Y-downward) xor (bitmap is Y-downward) and cfg->stencil_y_down = (bitmap
 * is Y-downward), as for msdfhip_generate: the two together tell the shape's orientation, and the stencil's memory row r is then the reference's --
 * row r of the SHAPE's rows for a Y-upward shape, row height-1-r for a Y-downward one, whatever the bitmap's own orientation (the legacy generators
 * re-orient the bitmap to the shape before they correct it, core/msdfgen.cpp:223). For the same reason the correction without sign_correction
 * walks the SHAPE's rows, as generateMSDF_legacy's does; with sign_correction it walks the bitmap's, as the CLI flow's does (main.cpp:1260-1294). */
int msdfhip_generate_legacy(int mode, float *pixels, int width, int height, int row_stride, int flip,
                            const int32_t *contour_offsets, int n_contours, const double *points, const uint8_t *types, const uint8_t *colors,
                            const double *xf, const MsdfHipConfig *cfg, uint8_t *stencil);
/* msdfErrorCorrection_legacy(output, threshold) on a 3- or 4-channel bitmap, in place: the clash detection between axial, then diagonal neighbours.
 *   replaces core/msdf-error-correction.cpp:115-181 (declared core/msdf-error-correction.h:37-38). Any row stride (in floats, may be negative). */
int msdfhip_error_correction_legacy(int channels, float *pixels, int width, int height, int row_stride, double threshold_x, double threshold_y);

/* distanceSignCorrection(sdf, shape, projection, sdfZeroValue, fillRule) on an existing 1-, 3- or 4-channel bitmap, in place.
 *   replaces core/rasterization.cpp:19-92 (declared core/rasterization.h:17-19; the legacy overloads :21-27 forward).
 * xf: only the Projection part {sx, sy, tx, ty} is read. fill_rule: FillRule (core/Scanline.h:10-15). */
int msdfhip_distance_sign_correction(int channels, float *pixels, int width, int height, int row_stride, int flip,
                                     const int32_t *contour_offsets, int n_contours, const double *points, const uint8_t *types, const uint8_t *colors,
                                     const double *xf, float sdf_zero_value, int fill_rule);

/* rasterize(output, shape, projection, fillRule): 1-channel coverage bitmap, 1.f where the texel centre is filled.
 *   replaces core/rasterization.cpp:8-16 (declared core/rasterization.h:13, legacy overload :22) -- the same scanline fill
 *   test as the sign correction; provided so that a build can drop the reference's rasterization.cpp as a whole. */
int msdfhip_rasterize(float *pixels, int width, int height, int row_stride, int flip,
                      const int32_t *contour_offsets, int n_contours, const double *points, const uint8_t *types, const uint8_t *colors,
                      const double *xf, int fill_rule);

/* Transparent micro-batching of the single-shape entry points above. Host threads that call them concurrently
 * (msdf-atlas-gen's workers) are combined group-commit style into one device batch per set of calls with equal launch parameters
 * (mode, config); sizes may differ within MSDFHIP_MICROBATCH_MAX_PAD: a leader takes queued calls in arrival order while the
 * group's padded grid n*W*H (W, H: the largest width and height taken) stays within that factor of the sum of the calls' own
 * w*h and the slot W*H within that factor of every member's own w*h, and runs them as one sized batch; below 1 (also 0) only calls of equal size share a group. The legacy generators
 * (msdfhip_generate_legacy) always group by equal size. A lone caller never waits. On by default (groups of up to 256 calls,
 * 4 concurrent leaders); the environment variable MSDFHIP_MICROBATCH=0 or max_group <= 1 turns it off (every call then runs on
 * its own stream).
 * msdfhip_microbatch_stats: calls served / device batches run / largest group since the last reset. */
int msdfhip_set_microbatch(int max_group, int max_leaders);
int msdfhip_microbatch_stats(long long *calls, long long *batches, long long *largest, int reset);
/* The groups among them that held bitmaps of different sizes, since the last reset: such groups / their calls / the sum of their
 * padded grids n*W*H / the sum of their calls' own w*h (texels). Any pointer may be NULL. */
int msdfhip_microbatch_mixed_stats(long long *mixed_batches, long long *mixed_calls, long long *padded_texels, long long *box_texels, int reset);
/* Makes grouping deterministic for tests and A/B scripts. hold_ms > 0: single-shape calls that arrive queue up and no new group
 * starts until the hold is released or hold_ms milliseconds have passed since this call (the wait is bounded: a hold that nobody
 * releases ends by itself); groups already running finish. hold_ms == 0: releases the hold. Returns the number of queued calls
 * that no group has taken yet (negative: an error code). Host state only: no device is touched. */
int msdfhip_microbatch_hold(int hold_ms);
/* Where the host-pointer calls spend their wall time, summed over device batches since the last reset (milliseconds):
 * staging the inputs, H2D + kernels + D2H + stream sync, scattering the tiles into the callers' bitmaps. */
int msdfhip_microbatch_times(double *stage_ms, double *device_ms, double *scatter_ms, int reset);

/* ShapeDistanceFinder<CC<Selector>>::oneShotDistance at n shape-space points (core/ShapeDistanceFinder.hpp:36-58; the
 * per-pixel engine under generate*).  selector = mode 1..4; out receives n*4 doubles (unused channels 0). */
int msdfhip_shape_distance(int selector, int overlap_support, const int32_t *contour_offsets, int n_contours, const double *points,
                           const uint8_t *types, const uint8_t *colors, int n_points, const double *pts, double *out);

/* ------------------------------------------------------------------------------------------------------------------
 * Batched, device-resident path (what an atlas generator uses): G glyph shapes -> G tiles of width x height.
 * "Upload once": the edge buffer is flattened by the caller, lives in HBM, and is pre-digested on the device into
 * per-edge records (end tangents, corner bisectors, polynomial coefficients, contour windings).
 * ------------------------------------------------------------------------------------------------------------------ */

typedef struct MsdfHipBatch MsdfHipBatch; /* opaque */

/* Creates a batch from HOST arrays (copied to the device; contour_offsets are global edge indices):
 *   glyph_contour_offsets int32[n_glyphs+1], contour_offsets int32[n_contours+1], points double[n_edges*8], types/colors uint8[n_edges]. */
int msdfhip_batch_create(MsdfHipBatch **batch, int n_glyphs, const int32_t *glyph_contour_offsets, const int32_t *contour_offsets,
                         const double *points, const uint8_t *types, const uint8_t *colors);
/* Same, on an explicit device (-1 = the process default). One host thread per device may create and run its own batch concurrently. */
int msdfhip_batch_create_on(MsdfHipBatch **batch, int device, int n_glyphs, const int32_t *glyph_contour_offsets, const int32_t *contour_offsets,
                            const double *points, const uint8_t *types, const uint8_t *colors);
int msdfhip_batch_device(const MsdfHipBatch *batch, int *device);
/* Same, from DEVICE arrays that already live in HBM (e.g. torch tensors); they must stay valid until the batch is destroyed.
 * max_contours_per_glyph / max_edges_per_glyph are host-known upper bounds used to size LDS. `stream` is a hipStream_t (or NULL). */
int msdfhip_batch_create_device(MsdfHipBatch **batch, int n_glyphs, int n_contours, int n_edges, int max_contours_per_glyph, int max_edges_per_glyph,
                                const int32_t *d_glyph_contour_offsets, const int32_t *d_contour_offsets,
                                const double *d_points, const uint8_t *d_types, const uint8_t *d_colors, void *stream);
/* Re-runs the on-device digestion (records + windings) on `stream`, e.g. after the caller rewrote the edge arrays in place
 * (device-array batches) -- this is the per-upload part of the pipeline that a benchmark step should include. */
int msdfhip_batch_digest(MsdfHipBatch *batch, void *stream);
void msdfhip_batch_destroy(MsdfHipBatch *batch);
/* Contour::winding (core/Contour.cpp:57-81) of every contour of the batch, as computed on the device (host int32[n_contours]). */
int msdfhip_batch_windings(const MsdfHipBatch *batch, int32_t *windings);

/* Generates all tiles of the batch: glyph g's tile is written at d_out + d_glyphs[g].out_offset with d_glyphs[g].row_stride.
 * d_glyphs (device, MsdfHipGlyph[n_glyphs]), d_out (device floats), d_stencil (device, n_glyphs*width*height bytes, or NULL),
 * d_scratch: device floats for the intermediate fields: one tile extent (n_glyphs*width*height*N) if error correction OR sign
 * correction runs, two if both do; may be NULL, then internal buffers are used.
 * Asynchronous on `stream` (hipStream_t or NULL = default stream). Replaces a loop of msdfgen.h:46-53 calls.
 * Thread safety: a batch keeps per-batch work buffers (candidate lists, bucket lists, the internal scratch); issue its calls from one
 * stream at a time. Different batches, and the single-shape entry points above, are independent of each other. */
int msdfhip_batch_generate(const MsdfHipBatch *batch, int mode, int width, int height, const MsdfHipGlyph *d_glyphs,
                           float *d_out, uint8_t *d_stencil, float *d_scratch, const MsdfHipConfig *cfg, void *stream);
/* msdfhip_batch_generate with a bitmap size PER GLYPH (a tightly packed atlas: every glyph's box is its bounds plus the pixel range).
 * sizes: HOST int32[n_glyphs*2] = w_g, h_g, each >= 1. Glyph g is generated as a w_g x h_g bitmap at d_out + d_glyphs[g].out_offset with
 * d_glyphs[g].row_stride; flip reverses ITS h_g rows. With W = max w_g, H = max h_g, "slot" = W*H texels:
 *   d_scratch  as msdfhip_batch_generate for a W x H call (n_glyphs*slot*N floats per intermediate field); glyph g's intermediate field is PACKED
 *              [h_g][w_g][N] at the start of slot g
 *   d_stencil  NULL or n_glyphs*slot bytes; glyph g's stencil is w_g*h_g bytes packed at g*slot, rows as msdfhip_batch_generate defines them
 * The result per glyph is what msdfhip_batch_generate writes for that glyph at width = w_g, height = h_g, the behaviour of the correction and sign
 * passes at the box's own borders included; the launches are those of a W x H call (same routes), workgroups outside a glyph's box leave at once.
 * The sizes are read before the call returns (the batch keeps its own device copy, ordered on `stream` in front of the first launch).
 * Fails with MSDFHIP_ERR_INVALID before the device is touched on sizes == NULL, any w_g, h_g < 1, or n_glyphs*slot beyond the 32-bit texel index. */
int msdfhip_batch_generate_sized(const MsdfHipBatch *batch, int mode, const int32_t *sizes, const MsdfHipGlyph *d_glyphs,
                                 float *d_out, uint8_t *d_stencil, float *d_scratch, const MsdfHipConfig *cfg, void *stream);
/* The legacy generators (msdfhip_generate_legacy above) for every glyph of the batch; arguments, scratch size and stream as msdfhip_batch_generate,
 * `cfg` read as msdfhip_generate_legacy reads it. The call leaves nothing on the batch that a later msdfhip_batch_generate would rely on. */
int msdfhip_batch_generate_legacy(const MsdfHipBatch *batch, int mode, int width, int height, const MsdfHipGlyph *d_glyphs,
                                  float *d_out, uint8_t *d_stencil, float *d_scratch, const MsdfHipConfig *cfg, void *stream);
/* msdfErrorCorrection_legacy of n_glyphs packed device tiles d_tiles[g][h][w][channels] (channels 3 or 4), in place; d_scratch: device floats, as
 * many as the tiles hold (the two passes run tiles -> scratch -> tiles). Asynchronous on `stream`. */
int msdfhip_batch_error_correction_legacy(float *d_tiles, int n_glyphs, int width, int height, int channels, float *d_scratch,
                                          double threshold_x, double threshold_y, void *stream);
/* End to end into HOST memory (what replaces an atlas generator's loop of generate*() calls into caller-owned bitmaps,
 * core/msdfgen.cpp:52-76, README.md:133): HOST descriptors, HOST output. The glyph list is processed in chunks on two streams, so the
 * kernels of one chunk overlap the device-to-host copy of the previous one; synchronous for the caller.
 *   glyphs[g].out_offset / row_stride place tile g in `out` (floats). A chunk whose rectangles exactly tile one contiguous range of
 *   `out` (tiles packed in glyph order; glyphs in row-major order filling whole row bands of an atlas) is written by the device in that
 *   layout and copied back as ONE contiguous copy; any other placement (gaps, negative strides) is copied into pinned staging and
 *   scattered row by row on the host while the next chunk runs -- texels outside the rectangles are never touched.
 *   stencil: NULL or n_glyphs*width*height bytes; written only when an error-correction pass runs (like the reference's buffer).
 * For full copy speed `out` should be pinned (msdfhip_host_alloc); pageable memory works, the runtime then stages the copies. */
int msdfhip_batch_generate_host(const MsdfHipBatch *batch, int mode, int width, int height, const MsdfHipGlyph *glyphs,
                                float *out, size_t out_floats, uint8_t *stencil, const MsdfHipConfig *cfg);
/* Same pipeline with 8-bit output: every chunk's float tiles stay on the device, are converted with pixelFloatToByte
 * (core/pixel-conversion.hpp:8-10) and blitted into the caller's uint8 atlas; glyphs[g].out_offset / row_stride are in BYTES of
 * `atlas`. The copy back is a quarter of the float tiles'. */
int msdfhip_batch_generate_bytes_host(const MsdfHipBatch *batch, int mode, int width, int height, const MsdfHipGlyph *glyphs,
                                      uint8_t *atlas, size_t atlas_bytes, const MsdfHipConfig *cfg);
/* STREAMED generation: shapes in, host bitmaps out, with everything in between overlapped -- SURVEY.md 8(d)'s end-to-end metric (host flatten + H2D +
 * kernels incl. error correction + D2H into caller bitmaps) as ONE pipelined call. The two-step form above (msdfhip_batch_create, then
 * msdfhip_batch_generate_host) flattens everything, uploads and digests everything, and only then starts the chunk pipeline; here the glyph list is cut
 * into the pipeline's chunks first and the library's host threads flatten chunk k+1 / k+2 straight into pinned staging WHILE chunk k is uploaded, digested and
 * rendered and chunk k-1 is copied back. Replaces a caller loop of generate*() calls over a list of shapes (core/msdfgen.cpp:52-76, README.md:133,
 * main.cpp:1243-1275); the C++ shim's msdfgen_hip::generate*Batch() are built on it.
 *
 * MsdfHipShapeSource: how the library reads the caller's shape objects (for msdfgen: `const Shape &`, core/Shape.h:15-58 -- contours[i].edges[j]->type(),
 * controlPoints(), color; core/edge-segments.h:28-31). Both callbacks are called from several library threads at once, each glyph exactly once per pass;
 * they must only READ the shapes.
 *   count(user, glyph, &n_contours, &n_edges)   cheap first pass over the whole list (sizes the chunks and the staging)
 *   fill(user, glyph, edge_base, contour_end, points, types, colors)
 *        contour_end int32[n_contours]: edge_base + the index one past contour c's last edge (edges of the glyph numbered from 0 in Shape order)
 *        points double[n_edges*8], types uint8[n_edges] (1 linear, 2 quadratic, 3 cubic), colors uint8[n_edges]: as for msdfhip_generate above
 *   The arrays handed to fill ARE the pinned staging: what fill writes is what the device reads, there is no intermediate copy.
 * device: -1 = the process default. glyphs / out / atlas / stencil / cfg: exactly as msdfhip_batch_generate_host / _bytes_host (exactly one of out, atlas). */
typedef struct MsdfHipShapeSource {
    void *user;
    void (*count)(void *user, int glyph, int32_t *n_contours, int32_t *n_edges);
    void (*fill)(void *user, int glyph, int32_t edge_base, int32_t *contour_end, double *points, uint8_t *types, uint8_t *colors);
} MsdfHipShapeSource;
int msdfhip_generate_stream(int device, int mode, int width, int height, int n_glyphs, const MsdfHipShapeSource *source, const MsdfHipGlyph *glyphs,
                            float *out, size_t out_floats, uint8_t *atlas, size_t atlas_bytes, uint8_t *stencil, const MsdfHipConfig *cfg);
/* The same pipeline over HOST CSR arrays (the arguments of msdfhip_batch_create): upload and digest go chunk by chunk under the kernels instead of in front. */
int msdfhip_generate_stream_csr(int device, int mode, int width, int height, int n_glyphs, const int32_t *glyph_contour_offsets, const int32_t *contour_offsets,
                                const double *points, const uint8_t *types, const uint8_t *colors, const MsdfHipGlyph *glyphs,
                                float *out, size_t out_floats, uint8_t *atlas, size_t atlas_bytes, uint8_t *stencil, const MsdfHipConfig *cfg);
/* Host threads of the streamed generator's flatten pool, incl. the calling thread (0 = the usable cores -- affinity mask and cgroup quota --, at most 32; also
 * MSDFHIP_HOST_THREADS). The pool is created on first use: returns 0 when the value was taken, else the size of the pool that already exists. */
int msdfhip_set_host_threads(int threads);
/* GPU_MAX_HW_QUEUES as the host process exported it (0: not set -- the HIP runtime then multiplexes all streams onto 4 hardware queues and the chunks of the
 * generators above wait behind one another's copies: 12.0 instead of 10.2 ms per 8 192 glyphs). The library does not touch the environment; a host that
 * runs the pipeline with fewer than 8 gets ONE note on stderr if MSDFHIP_VERBOSE is set (a drop-in library stays silent by default). Figures in README.md / DESIGN.md assume GPU_MAX_HW_QUEUES=8. */
int msdfhip_hw_queues_env(void);
/* How often a host-output / streamed call was run a second time because a glyph's distance-check candidates overflowed their segment (more than 1/16 of its
 * texels needed a check: overlapping strokes rendered without overlap support, ALWAYS_CHECK_DISTANCE on noise). The chunks of those calls do not launch the
 * per-texel overflow pass; the count is mirrored to the host with the chunk's results and such a call is repeated with the pass -- same bytes either way. */
unsigned long long msdfhip_pipeline_overflow_reruns(int reset);
/* Glyphs per pipeline chunk (0 = automatic: about 96 MB of float tiles). */
int msdfhip_set_pipeline_chunk(int glyphs_per_chunk);
/* Pinned (page-locked, portable across devices) host memory for outputs of the two functions above. */
int msdfhip_host_alloc(void **p, size_t bytes);
int msdfhip_host_free(void *p);

/* Glyph-sharded generation on several devices of one node: the glyph list (HOST CSR arrays as for
 * msdfhip_batch_create) is cut into n_devices contiguous ranges balanced by edge count; one host thread per entry of `devices`
 * uploads its range, runs the pipeline above on that device and copies its tiles straight into the caller's buffer. No exchange
 * between devices; the bytes do not depend on the split (a device may be listed more than once), and any tile placement is fine: a
 * device only ever writes its own glyphs' rectangles. Exactly one of `out` (float tiles, offsets in floats) and `atlas` (8-bit,
 * offsets in bytes) is non-NULL. */
int msdfhip_generate_sharded(const int *devices, int n_devices, int mode, int width, int height, int n_glyphs,
                             const int32_t *glyph_contour_offsets, const int32_t *contour_offsets, const double *points, const uint8_t *types,
                             const uint8_t *colors, const MsdfHipGlyph *glyphs, float *out, size_t out_floats, uint8_t *atlas, size_t atlas_bytes,
                             const MsdfHipConfig *cfg);

/* Shape preparation on the device: what callers run on every glyph before the generators.
 *   normalize  Shape::normalize (core/Shape.cpp:65-92): single-edge contours split in thirds, convergent edges pushed apart
 *   coloring   0 keep `colors`, 1 edgeColoringSimple(shape, angle_threshold, seed) (core/edge-coloring.cpp:68-142),
 *              2 edgeColoringInkTrap(shape, angle_threshold, seed) (core/edge-coloring.cpp:151-258)
 * msdfhip_batch_create_prepared uploads RAW outlines (colors may be NULL = all WHITE), prepares them on the device and returns a
 * digested batch of the prepared shapes; seeds: one per glyph, or NULL to use cfg->seed for every glyph. The prepared shapes can be
 * read back with msdfhip_batch_info (sizes) + msdfhip_batch_download (arrays sized from those; any pointer may be NULL). */
typedef struct MsdfHipPrepConfig {
    int32_t normalize;
    int32_t coloring;
    double angle_threshold;       /* main.cpp:32: 3.0 */
    uint64_t seed;
} MsdfHipPrepConfig;
int msdfhip_batch_create_prepared(MsdfHipBatch **batch, int n_glyphs, const int32_t *glyph_contour_offsets, const int32_t *contour_offsets,
                                  const double *points, const uint8_t *types, const uint8_t *colors, const uint64_t *seeds,
                                  const MsdfHipPrepConfig *cfg);
/* The streamed generator (msdfhip_generate_stream / _csr) over RAW outlines: every chunk is uploaded, prepared on the device (prep, seeds: as for
 * msdfhip_batch_create_prepared), digested, rendered and copied back on its own stream, overlapped with the neighbouring chunks. The bytes of glyph g are
 * those of msdfhip_batch_create_prepared with the same arrays, prep and seeds followed by msdfhip_batch_generate_host / _bytes_host, whatever the chunks.
 * Source form: the colours `fill` writes are used only when prep->coloring == 0. CSR form: colors may be NULL (all WHITE).
 * A NULL prep, a coloring outside 0..2 or a stencil with atlas output fail with MSDFHIP_ERR_INVALID before the device is touched. */
int msdfhip_generate_stream_prepared(int device, int mode, int width, int height, int n_glyphs, const MsdfHipShapeSource *source,
                                     const MsdfHipGlyph *glyphs, float *out, size_t out_floats, uint8_t *atlas, size_t atlas_bytes,
                                     uint8_t *stencil, const MsdfHipConfig *cfg, const MsdfHipPrepConfig *prep, const uint64_t *seeds);
int msdfhip_generate_stream_csr_prepared(int device, int mode, int width, int height, int n_glyphs, const int32_t *glyph_contour_offsets,
                                         const int32_t *contour_offsets, const double *points, const uint8_t *types, const uint8_t *colors,
                                         const MsdfHipGlyph *glyphs, float *out, size_t out_floats, uint8_t *atlas, size_t atlas_bytes,
                                         uint8_t *stencil, const MsdfHipConfig *cfg, const MsdfHipPrepConfig *prep, const uint64_t *seeds);
/* Orientation around the preparation above, in the reference CLI's order:
 *   orient_contours  1: Shape::orientContours (core/Shape.cpp:144-198) on the raw outline, before normalize (main.cpp:1105-1111, -windingpreprocess)
 *   winding          after normalize, before the colouring (main.cpp:1131-1143): 0 keep, 1 reverse every contour (-reversewinding),
 *                    2 reverse every contour when the true distance at a point outside Shape::getBounds is positive (-guesswinding)
 * The _oriented entry points are their twins above plus `orient`; NULL means keep (what the twins do). Edge and contour counts do not change.
 * orient_contours outside 0..1 or winding outside 0..2 fail with MSDFHIP_ERR_INVALID before the shape source is read or the device is touched. */
typedef struct MsdfHipOrientConfig {
    int32_t orient_contours;
    int32_t winding;              /* 0 keep, 1 reverse, 2 guess */
} MsdfHipOrientConfig;
int msdfhip_batch_create_prepared_oriented(MsdfHipBatch **batch, int n_glyphs, const int32_t *glyph_contour_offsets, const int32_t *contour_offsets,
                                           const double *points, const uint8_t *types, const uint8_t *colors, const uint64_t *seeds,
                                           const MsdfHipPrepConfig *cfg, const MsdfHipOrientConfig *orient);
int msdfhip_generate_stream_prepared_oriented(int device, int mode, int width, int height, int n_glyphs, const MsdfHipShapeSource *source,
                                              const MsdfHipGlyph *glyphs, float *out, size_t out_floats, uint8_t *atlas, size_t atlas_bytes,
                                              uint8_t *stencil, const MsdfHipConfig *cfg, const MsdfHipPrepConfig *prep, const uint64_t *seeds,
                                              const MsdfHipOrientConfig *orient);
int msdfhip_generate_stream_csr_prepared_oriented(int device, int mode, int width, int height, int n_glyphs, const int32_t *glyph_contour_offsets,
                                                  const int32_t *contour_offsets, const double *points, const uint8_t *types, const uint8_t *colors,
                                                  const MsdfHipGlyph *glyphs, float *out, size_t out_floats, uint8_t *atlas, size_t atlas_bytes,
                                                  uint8_t *stencil, const MsdfHipConfig *cfg, const MsdfHipPrepConfig *prep, const uint64_t *seeds,
                                                  const MsdfHipOrientConfig *orient);
/* Framing on the device: Shape::getBounds (core/Shape.cpp:104-115, without border / miters) and what the reference CLI's -autoframe makes of it
 * (main.cpp:1153-1183), per glyph, so that a caller hands over outlines and ONE tile size instead of a transformation per glyph.
 *   range_mode / range_lower / range_upper   the CLI's -range / -arange (0: in shape units) or -pxrange / -apxrange (1: in pixels of the tile)
 *   scale_specified                          0: the glyph is fitted into width x height (less the pixel range); 1: centred at scale_x / scale_y (-scale)
 * A glyph whose bounds are empty (l >= r or b >= t: no edges, a single vertical or horizontal line) is framed as the unit box, like the CLI.
 * The bounds are those of the NORMALIZED shape, before any colouring (main.cpp:1125-1132): batches made by msdfhip_batch_create_prepared[_oriented] took
 * them at that point; batches made from arrays that are prepared already take them from those arrays.
 * A frame that cannot fit ("Cannot fit the specified pixel range", main.cpp:1164: width or height + 2*range_lower <= 0 for a pixel range without a given
 * scale), a range_mode outside 0..1, range_lower == range_upper and scale_specified with a zero scale fail with MSDFHIP_ERR_INVALID before anything is read
 * or the device is touched. */
typedef struct MsdfHipFrameConfig {
    int32_t range_mode;        /* 0 unit range (-range / -arange), 1 pixel range (-pxrange / -apxrange) */
    int32_t scale_specified;   /* 0: fit the glyph (autoframe picks scale); 1: centre it at scale_x / scale_y */
    double range_lower, range_upper;
    double scale_x, scale_y;
} MsdfHipFrameConfig;
/* Shape::getBounds of every glyph of the batch: host double[n_glyphs*4] = l, b, r, t (an empty glyph: 1e240, 1e240, -1e240, -1e240). Synchronous. */
int msdfhip_batch_bounds(const MsdfHipBatch *batch, double *bounds);
/* Writes xf[0..5] of d_glyphs[g] (device, MsdfHipGlyph[n_glyphs]) for a width x height tile; out_offset, row_stride and flip stay as the caller set them.
 * Asynchronous on `stream`; msdfhip_batch_generate with the same d_glyphs on that stream follows without a host round trip. */
int msdfhip_batch_frame(const MsdfHipBatch *batch, const MsdfHipFrameConfig *frame, int width, int height, MsdfHipGlyph *d_glyphs, void *stream);
/* The streamed generators over raw outlines with framing: with `frame` the xf of the host glyphs[] are ignored and every chunk is framed on its own stream
 * between its preparation and its digest; frame == NULL is the twin above. Same bytes as the twin given the xf that msdfhip_batch_frame writes. */
int msdfhip_generate_stream_prepared_oriented_framed(int device, int mode, int width, int height, int n_glyphs, const MsdfHipShapeSource *source,
                                                     const MsdfHipGlyph *glyphs, float *out, size_t out_floats, uint8_t *atlas, size_t atlas_bytes,
                                                     uint8_t *stencil, const MsdfHipConfig *cfg, const MsdfHipPrepConfig *prep, const uint64_t *seeds,
                                                     const MsdfHipOrientConfig *orient, const MsdfHipFrameConfig *frame);
int msdfhip_generate_stream_csr_prepared_oriented_framed(int device, int mode, int width, int height, int n_glyphs, const int32_t *glyph_contour_offsets,
                                                         const int32_t *contour_offsets, const double *points, const uint8_t *types, const uint8_t *colors,
                                                         const MsdfHipGlyph *glyphs, float *out, size_t out_floats, uint8_t *atlas, size_t atlas_bytes,
                                                         uint8_t *stencil, const MsdfHipConfig *cfg, const MsdfHipPrepConfig *prep, const uint64_t *seeds,
                                                         const MsdfHipOrientConfig *orient, const MsdfHipFrameConfig *frame);
/* Box sizes on the device: Shape::getBounds(border, miterLimit, polarity) WITH border and miters (core/Shape.cpp:99-115, core/Contour.cpp:39-55), and from
 * it the box an atlas generator gives every glyph at one common scale -- its size in texels and the transformation that puts the glyph into it -- so that
 * the field of a sharp corner is not cut off by the box edge and the caller never walks the geometry on the host.
 * Which arrays the two parts read: the plain bounds are those of msdfhip_batch_bounds (batches made by msdfhip_batch_create_prepared[_oriented]: fixed after
 * their normalize); the miters are taken over the edges the batch HOLDS (for such a batch the oriented, coloured ones) -- what a caller gets who keeps
 * getBounds() from load time and calls Shape::boundMiters on the shape it is about to render. For batches made from prepared arrays that is exactly
 * getBounds(border, miter_limit, polarity) of those arrays, bit for bit. The reference's gates stay: nothing changes unless border > 0, no miter is taken
 * unless also miter_limit > 0; no argument is invalid. Host double[n_glyphs*4] = l, b, r, t. Synchronous. */
int msdfhip_batch_bounds_miters(const MsdfHipBatch *batch, double border, double miter_limit, int polarity, double *bounds);
/* The boxes. With s = scale, (lo, hi) = the range in shape units (a pixel range: range_lower/s, range_upper/s) and l, b, r, t the bounds above with
 * border = -lo, per axis (l, r -> w, tx; b, t -> h, ty):
 *   aligned (the texel grid passes through the shape's origin)   sl = floor(s*l - .5), sr = ceil(s*r + .5): w = sr - sl, tx = -sl/s
 *   otherwise (the glyph is centred)                             d = s*(r - l): w = ceil(d) + 1, tx = -l + (.5*(w - d))/s
 * and xf[g] = s, s, tx, ty, 1/(hi - lo), -lo: the six doubles of MsdfHipGlyph.xf as they are. A glyph whose PLAIN bounds are empty (l >= r or b >= t: no
 * edges, a lone horizontal or vertical line) has no box: sizes 0 x 0, tx = ty = 0 -- msdfhip_batch_generate_sized wants at least 1 x 1, so give such a
 * glyph one texel or leave it out. sizes: host int32[n_glyphs*2] = w, h; xf: host double[n_glyphs*6]; bounds: host double[n_glyphs*4], the extended bounds,
 * or NULL. Synchronous. A bad field of the config fails with MSDFHIP_ERR_INVALID before the device is touched; so does, after the launch, a box with a side
 * that is not a number or beyond 2^30 texels (nothing is written then). */
typedef struct MsdfHipBoxConfig {
    double scale;                      /* texels per shape unit, both axes; > 0, finite */
    int32_t range_mode;                /* 0 unit range, 1 pixel range */
    double range_lower, range_upper;   /* lower < upper, lower <= 0, finite */
    double miter_limit;                /* <= 0: no miters */
    int32_t polarity;                  /* as Contour::boundMiters: > 0 / < 0 only the corners turning one way, 0 every corner */
    int32_t align_x, align_y;          /* 0 or 1: pixel-align the origin per axis */
} MsdfHipBoxConfig;
int msdfhip_batch_boxes(const MsdfHipBatch *batch, const MsdfHipBoxConfig *cfg, int32_t *sizes, double *xf, double *bounds);
/* Diagnostics: after an error-correction pass, counts[0] = 1 if some glyph's candidate segment overflowed (those glyphs were redone by
 * the full per-texel pipeline), counts[1+g] = deferred distance checks pushed for glyph g. counts holds n_glyphs+1 entries. */
int msdfhip_batch_candidate_counts(const MsdfHipBatch *batch, uint32_t *counts);
int msdfhip_batch_info(const MsdfHipBatch *batch, int *n_glyphs, int *n_contours, int *n_edges, int *max_contours, int *max_edges);
int msdfhip_batch_download(const MsdfHipBatch *batch, int32_t *contour_offsets, double *points, uint8_t *types, uint8_t *colors);
/* A new batch out of glyphs that are already resident (a dynamic atlas taking some glyphs of a font, several fonts in one atlas, one glyph under several
 * transformations, the glyphs of one box-size class): glyph k of the result is glyph indices[k] of sources[source_of[k]].
 *   sources    HOST array of n_sources batches on one device; source_of, indices: HOST int32[n_glyphs], read before the call returns.
 *              source_of == NULL: every glyph comes from sources[0] (n_sources must then be 1). Indices may repeat, come in any order and leave glyphs
 *              out; n_glyphs == 0 gives an empty batch.
 * The result's arrays are those msdfhip_batch_create would hold for the chosen shapes in that order (offsets rebased; points, types, colours edge for
 * edge), copied on the device and digested like any new batch; msdfhip_batch_info reports the counts and per-glyph maxima of the SELECTION. It owns all
 * of them: a source may be destroyed, digested again or rewritten as soon as the call has returned (destroying it frees device memory, which waits for
 * the device). Bounds: if a source has the bounds it took at creation (msdfhip_batch_create_prepared*), the result keeps, per glyph, the bounds of the
 * glyph's source (computed on `stream` for a source that has none fixed); otherwise the result computes them on demand from its own arrays.
 * Asynchronous on `stream`: the upload of the copy plan (from pinned memory the result keeps), the copies and the digestion are ordered on it, so the
 * points, types and colours of a source may still be pending there; its OFFSETS are read when the call is made (first need of the per-glyph counts of
 * a msdfhip_batch_create_device batch: one synchronous read-back), and allocations may wait for the device. Caller's arrays under such a source stay
 * valid until `stream` has passed the call.
 * Fails with MSDFHIP_ERR_INVALID, naming the position, before anything is allocated or launched: batch, sources or an entry of it NULL; n_sources < 1;
 * n_glyphs < 0; indices NULL with n_glyphs > 0; source_of NULL with n_sources > 1; a source_of[k] outside 0..n_sources-1; an index outside its
 * source's glyphs; sources on different devices; more than INT32_MAX contours or edges in all (summed in 64 bits: instancing reaches that). */
int msdfhip_batch_gather(MsdfHipBatch **batch, const MsdfHipBatch *const *sources, int n_sources, int n_glyphs, const int32_t *source_of,
                         const int32_t *indices, void *stream);

/* 8-bit atlas output: converts packed fp32 tiles [g][h][w][channels] (msdfhip_batch_generate's output with out_offset =
 * g*h*w*channels, row_stride = w*channels) with pixelFloatToByte (core/pixel-conversion.hpp:8-10, what the reference's savers
 * apply, core/save-bmp.cpp:174-224, ext/save-png.cpp:83-187) and stores glyph g's rectangle at
 * d_atlas + d_glyphs[g].out_offset + d_glyphs[g].row_stride*y + channels*x, offsets and strides in BYTES (xf and flip are not read).
 * Asynchronous on `stream`. The device-to-host copy of an 8-bit atlas is a quarter of the float tiles'. */
int msdfhip_tiles_to_bytes(const float *d_tiles, int n_glyphs, int width, int height, int channels, const MsdfHipGlyph *d_glyphs,
                           uint8_t *d_atlas, void *stream);
/* msdfhip_tiles_to_bytes for boxes: d_tiles holds glyph g packed [h_g][w_g][channels] at float offset tile_offsets[g] (HOST int64[n_glyphs]);
 * sizes as msdfhip_batch_generate_sized (HOST int32[n_glyphs*2], validated the same way before the device is touched). The conversion is ordered on
 * `stream`; the call returns when it has run (the device copy of the two host arrays lives for the call: there is no batch to keep it). */
int msdfhip_tiles_to_bytes_sized(const float *d_tiles, int n_glyphs, const int32_t *sizes, const int64_t *tile_offsets, int channels,
                                 const MsdfHipGlyph *d_glyphs, uint8_t *d_atlas, void *stream);

/* estimateSDFError(sdf, shape, projection, scanlinesPerRow, fillRule) for every glyph of a batch: d_errors[g] from the
 * packed tiles d_tiles[g][h][w][channels] (memory rows; what msdfhip_batch_generate wrote), without leaving the device.
 *   replaces core/sdf-error-estimation.cpp:134-164 (declared core/sdf-error-estimation.h:18-20).
 * d_glyphs[g].xf[0..3] = the Projection; d_glyphs[g].flip is read as "shape.getYAxisOrientation() == Y_DOWNWARD"
 * (sdf-error-estimation.cpp:146; for Y-upward bitmaps that is the flip flag the tiles were generated with). Asynchronous on `stream`. */
int msdfhip_batch_estimate_sdf_error(const MsdfHipBatch *batch, int channels, int width, int height, const MsdfHipGlyph *d_glyphs, const float *d_tiles,
                                     int scanlines_per_row, int fill_rule, double *d_errors, void *stream);
/* msdfhip_batch_estimate_sdf_error for boxes: glyph g's field is w_g x h_g, packed [h_g][w_g][channels] at float offset tile_offsets[g] of d_tiles (HOST
 * int64[n_glyphs]; what msdfhip_batch_generate_sized writes by default), sizes as that call takes them (HOST int32[n_glyphs*2] = w_g, h_g, validated the same
 * way, with the same texts, before the device is touched). d_errors[g] is what msdfhip_batch_estimate_sdf_error writes for glyph g alone at width = w_g,
 * height = h_g, bit for bit: (h_g-1)*scanlines_per_row scanlines, and 0 without any where w_g <= 1 or h_g <= 1 (core/sdf-error-estimation.cpp:136);
 * scanlines_per_row < 1 zeroes all errors. d_glyphs[g].xf[0..3] and .flip are read as there. channels outside {1, 3, 4}, fill_rule outside 0..3 or more than
 * 2^48 scanlines fail with MSDFHIP_ERR_INVALID. The work is ordered on `stream`; the call returns when it has run: the two host arrays are read before it
 * returns, and their device copy lives for the call, in the batch's list workspace beside the lists (calls on one batch are ordered by the caller, as ever).
 * MSDFHIP_ERROR_WORKSPACE_MB ("environment") caps the lists of one launch, of this call and of the uniform one. */
int msdfhip_batch_estimate_sdf_error_sized(const MsdfHipBatch *batch, int channels, const int32_t *sizes, const int64_t *tile_offsets,
                                           const MsdfHipGlyph *d_glyphs, const float *d_tiles, int scanlines_per_row, int fill_rule, double *d_errors, void *stream);

/* renderSDF(output, sdf, sdfPxRange, sdThreshold) for n_glyphs packed tiles: d_out[g][oh][ow][out_channels] from
 * d_sdf[g][sh][sw][sdf_channels], memory rows as they are.
 *   replaces core/render-sdf.cpp:14-170 (declared core/render-sdf.h:12-17); channel pairs as the reference's overloads:
 *   1<-1, 3<-1, 1<-3, 3<-3, 1<-4, 4<-4. range_lower == range_upper selects the thresholded rendering (core/render-sdf.cpp:16-23).
 * msdfhip_simulate_8bit: simulate8bit (core/render-sdf.cpp:172-188) on n floats in place. Both asynchronous on `stream`. */
int msdfhip_render_sdf(const float *d_sdf, int n_glyphs, int sdf_width, int sdf_height, int sdf_channels, float *d_out, int out_width, int out_height,
                       int out_channels, double range_lower, double range_upper, float sd_threshold, void *stream);
int msdfhip_simulate_8bit(float *d_pixels, size_t n, void *stream);
/* msdfhip_render_sdf for boxes: glyph g's sw_g x sh_g field, packed [sh_g][sw_g][sdf_channels] at float offset sdf_offsets[g] of d_sdf, is rendered into an
 * ow_g x oh_g bitmap packed [oh_g][ow_g][out_channels] at float offset out_offsets[g] of d_out -- renderSDF of that field into a bitmap of that size, bit for
 * bit: scale = (sw_g/ow_g, sh_g/oh_g) and the range times (ow_g+oh_g)/(sw_g+sh_g) PER GLYPH (core/render-sdf.cpp:16, 26), computed on the host in fp64 in the
 * order msdfhip_render_sdf computes them. sdf_sizes: HOST int32[n_glyphs*2] = sw_g, sh_g, validated as the sizes of msdfhip_tiles_to_bytes_sized are (same
 * texts, before the device is touched); out_sizes: HOST int32[n_glyphs*2] = ow_g, oh_g, where either side may be 0: that glyph writes nothing and its field is
 * not read; the two offset arrays: HOST int64[n_glyphs]. Channel pairs, range and threshold as msdfhip_render_sdf. The rendering is ordered on `stream`; the
 * call returns when it has run: the four host arrays are read before it returns (their device copy lives for the call: there is no batch to keep it). */
int msdfhip_render_sdf_sized(const float *d_sdf, int n_glyphs, const int32_t *sdf_sizes, const int64_t *sdf_offsets, int sdf_channels, float *d_out,
                             const int32_t *out_sizes, const int64_t *out_offsets, int out_channels, double range_lower, double range_upper, float sd_threshold,
                             void *stream);
/* The same two on HOST bitmaps (what the C++ shim's renderSDF / simulate8bit overloads call; synchronous). Strides in floats. */
int msdfhip_render_sdf_host(float *out, int out_width, int out_height, int out_row_stride, int out_channels,
                            const float *sdf, int sdf_width, int sdf_height, int sdf_row_stride, int sdf_channels,
                            double range_lower, double range_upper, float sd_threshold);
int msdfhip_simulate_8bit_host(float *pixels, int width, int height, int row_stride, int channels);

/* Timing hook for bench.py: average device time in milliseconds of the dominant kernel (the distance-field kernel) and of
 * the passes after it (sign correction + error correction, per error-correction launch) over the launches recorded since the
 * last call with reset != 0, measured with hipEvents on the launching stream.
 * Enable with msdfhip_set_kernel_timing(1) (adds two event records per launch). */
int msdfhip_set_kernel_timing(int enable);
int msdfhip_kernel_timing(double *avg_ms_distance, double *avg_ms_correction, int *launches, int reset);

/* Frees the pooled resources of the host-pointer entry points (arenas of the single-shape calls, pipelines of the host-output calls) that are
 * not in use right now. The pools grow to the peak number of concurrent calls and are otherwise kept for the life of the process. */
int msdfhip_trim(void);

/* MSDFHIP_DEVICES = "all" | "0,1,...": the devices over which the host-pointer single-shape entry points (msdfhip_generate* etc., and with them
 * the C++ shim) spread their micro-batched groups, round robin; unset = the default device (msdfhip_init). Returns how many are configured
 * and writes up to `cap` of them to `out`. */
int msdfhip_front_door_devices(int *out, int cap);

/* The library reads its MSDFHIP_* environment knobs ("environment") once, at first use. Tests and A/B scripts that change
 * the environment of a running process call this to have them read again. Not meant for production code. */
int msdfhip_reload_tuning(void);
/* Measurement builds only: the per-wavefront cycle table of the distance kernel (-DMSDF_PROFILE_WAITS, tools/profile_waits.py) or of the
 * distance checks of the error correction (-DMSDF_PROFILE_QUERY, tools/profile_query.py; reset = 2 reads its second page); a regular build
 * reports zeros. out24: 24 counters. reset = 1 clears the table after reading. */
int msdfhip_debug_wait_profile(unsigned long long *out24, int reset);
/* Measurement builds only (tools/isa_bbcount.py: -DMSDF_BBCOUNT, counter bumps inserted into the kernels' gfx950 assembly): execution counts per basic block of
 * the instrumented kernels since the last reset. Returns the number of counters written to `out` (at most `cap`); a regular build returns 0. */
int msdfhip_debug_bbcount(unsigned *out, int cap, int reset);
/* Fused single-shape launches (k_single_call): out8[0] = calls since the last reset (+ 1e-6 x the shader clock in MHz the launches ran at), out8[1..6] = microseconds per call, as seen by workgroup 0, of:
 * digest | its own distance tile | waiting for all tiles (grid barrier) | its own correction sweep | waiting for all sweeps | distance checks,
 * out8[7] = start of workgroup 0 to the last workgroup's end. Diagnostics (tools/host_call_latency.py). */
int msdfhip_debug_single_call_phases(double *out8, int reset);

/* The one-launch form of a single-shape call (k_single_call) needs all its workgroups resident at once. Calls that would not fit next to the fused
 * launches already in flight take the batched launch sequence instead (*refused); a launch that still finds the device occupied -- a persistent
 * kernel of another thread or process holds the slots -- gives up at its grid barrier after a bounded wait (*barrier_timeouts) and is rerun through the
 * batched sequence, as is one that ended without its completion flag (*lost_flags). The caller's generate*() succeeds either way
 * (core/msdfgen.cpp:78-106 cannot fail); these counters only say how often the slow road was taken since the last reset. Any pointer may be NULL. */
int msdfhip_single_call_fallbacks(unsigned long long *barrier_timeouts, unsigned long long *lost_flags, unsigned long long *refused, int reset);

/* Which launch route the batched passes took (tests: the routes depend on the size of a launch and on the MSDFHIP_* knobs). One relaxed counter per
 * launch site, bumped on the host when the launch is issued; a one-glyph batch beyond the small route counts in the class of its glyph.
 * Distance pass (dispatchDistance):
 *   0 SMALL_SIMPLE      small launch (<= MSDFHIP_SMALL_LAUNCH_TILES tiles), one tile per wavefront, simple combiner (also its one-contour part)
 *   1 SMALL_OVERLAP     small launch, overlapping combiner, combiner scratch in the global workspace
 *   2 ONE_QUAD          one-contour class, four tiles per wavefront
 *   3 ONE_SINGLE        one-contour class, one tile per wavefront (short launch)
 *   4 LDS_QUAD          LDS-scratch class, four tiles per wavefront
 *   5 LDS_SINGLE        LDS-scratch class, one tile per wavefront (short launch or MSDFHIP_LDS_CLASS_TPW=1)
 *   6 GLOBAL_DIRECT     global-scratch class, one workgroup per tile (chunked by workspace)
 *   7 GLOBAL_PERSISTENT global-scratch class, persistent workgroups drawing tiles from a work queue
 *   8 FULL_SIMPLE       the whole batch (or all but its oversized glyphs) through the four-tile simple-combiner plan, outside the small route
 *   9 UNCULLED          the list-free kernel (glyphs whose survivor lists exceed a CU's LDS)
 * Error correction (launchEc):
 *  10 EC_QUERY_HEAVIEST k_ec_query over the heaviest-first work list (batches of >= 256 glyphs)
 *  11 EC_QUERY_BATCH    k_ec_query in batch order
 *  12 EC_WIDE_SLOTS     the launch took the wide slot cap (up to 1 024 edges; batches of < 256 glyphs)
 *  13 EC_SLOW_ALL       k_ec_slow over every texel (more contours than k_ec_query's LDS scratch holds)
 * Sign pass (launchSign):
 *  14 SIGN_WHOLE_ROWS   a wavefront takes whole tile rows (span == tiles per row)
 *  15 SIGN_SPLIT        tile rows split between wavefronts
 *  16 SIGN_CHUNKED      the row lists hold fewer than 3 x the largest glyph's edges: edges walked in chunks
 * Writes min(cap, MSDFHIP_ROUTE_COUNT) counters to `out` and returns that number; reset != 0 zeroes all of them after reading. Diagnostics. */
#define MSDFHIP_ROUTE_DIST_SMALL_SIMPLE      0
#define MSDFHIP_ROUTE_DIST_SMALL_OVERLAP     1
#define MSDFHIP_ROUTE_DIST_ONE_QUAD          2
#define MSDFHIP_ROUTE_DIST_ONE_SINGLE        3
#define MSDFHIP_ROUTE_DIST_LDS_QUAD          4
#define MSDFHIP_ROUTE_DIST_LDS_SINGLE        5
#define MSDFHIP_ROUTE_DIST_GLOBAL_DIRECT     6
#define MSDFHIP_ROUTE_DIST_GLOBAL_PERSISTENT 7
#define MSDFHIP_ROUTE_DIST_FULL_SIMPLE       8
#define MSDFHIP_ROUTE_DIST_UNCULLED          9
#define MSDFHIP_ROUTE_EC_QUERY_HEAVIEST     10
#define MSDFHIP_ROUTE_EC_QUERY_BATCH        11
#define MSDFHIP_ROUTE_EC_WIDE_SLOTS         12
#define MSDFHIP_ROUTE_EC_SLOW_ALL           13
#define MSDFHIP_ROUTE_SIGN_WHOLE_ROWS       14
#define MSDFHIP_ROUTE_SIGN_SPLIT            15
#define MSDFHIP_ROUTE_SIGN_CHUNKED          16
#define MSDFHIP_ROUTE_COUNT                 17
int msdfhip_debug_route_counts(unsigned long long *out, int cap, int reset);

#ifdef __cplusplus
}
#endif
#endif /* MSDFGEN_HIP_H */
