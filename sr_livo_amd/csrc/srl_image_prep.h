// srl_image_prep.h -- internal: the image preparer's state (srl_image_prep.hip), read by srl_flow.hip (srl_flow_track_prepared takes
// d_gray_eq as its image).  Every plane has room for the pixel count rounded up to a multiple of 4 (k_prep_pixel, k_prep_apply).
#pragma once
#include "srl_ctx.h"

struct SrlImagePrep {
    srl_image_prep_opts opts;
    int rows = 0, cols = 0;
    int T = 0, tw = 0, th = 0, ext_rows = 0, ext_cols = 0;      // tiles per side, tile size, the (possibly) extended plane
    int limit[2] = {0, 0};                                      // clip limit of a tile's bins: [0] gray, [1] Y
    bool have_image = false;
    SrlImagePair raw;                                           // the upload: rows x cols x 3, rows packed
    char *d_block = nullptr;                                    // everything below: one block, laid out by prep_layout (srl_image_prep.hip)
    short *d_map1 = nullptr;                                    // (sx, sy) per pixel
    unsigned short *d_map2 = nullptr;                           // ay * 32 + ax per pixel
    unsigned char *d_undist = nullptr, *d_gray = nullptr, *d_y = nullptr, *d_crcb = nullptr;      // 3, 1, 1, 2 bytes per pixel
    unsigned char *d_lut = nullptr;                             // [plane][ty][tx][256]: plane 0 gray, 1 Y
    unsigned char *d_gray_eq = nullptr, *d_bgr_eq = nullptr;    // the two results
    // srl_image_prepare_resized: a frame of another size is uploaded into src and resized into raw.d
    SrlImagePair src;                                           // src_rows x src_cols x 3, rows packed; comes with the first such frame
    int *d_ofs_x = nullptr, *d_ofs_y = nullptr;                 // srl_image_resize_build_tables per column and per row of the preparer's size
    unsigned *d_coef_x = nullptr, *d_coef_y = nullptr;          // (coef[2 d], coef[2 d + 1]) as one dword
    int tab_rows = 0, tab_cols = 0;                             // the source size the tables on the device are for (0: none yet)
    const unsigned char *d_frame = nullptr;                     // the frame the last chain's remap read: raw.d, or a decoded JPEG frame where it lies
};

// four consecutive pixels of the image taken as one flat array per lane (k_prep_pixel, k_prep_apply, k_resize_bgr, k_jpeg_color)
struct PrepDims { int rows, cols, npix; };
// pixel 4 g + k of the flat image; beyond the image: the last pixel again
__device__ __forceinline__ void prep_first(const PrepDims &D, int g, int *x, int *y) {
    long long i = (long long)g * 4;
    if (i >= D.npix) i = D.npix - 1;
    *y = (int)(i / D.cols);
    *x = (int)(i - (long long)*y * D.cols);
}
__device__ __forceinline__ void prep_step(const PrepDims &D, int *x, int *y) {
    if (++*x == D.cols) { *x = 0; ++*y; }
    if (*y >= D.rows) { *y = D.rows - 1; *x = D.cols - 1; }
}

// the refusals of the preparer's entry points and of srl_flow_track_prepared: no preparer, no image yet; more than one rank
inline int srl_prep_need(srl_ctx *ctx, bool image) {
    if (!ctx->prep) { ctx->err = "no image preparer (srl_image_prep_create)"; return SRL_ERR_NO_MAP; }
    if (image && !ctx->prep->have_image) { ctx->err = "image preparer: no image yet (srl_image_prepare)"; return SRL_ERR_NO_SWEEP; }
    return SRL_OK;
}
inline int srl_prep_one_rank(srl_ctx *ctx) {
    if (ctx->nranks > 1) { ctx->err = "the image preparer is neither replicated nor sharded: one rank only"; return SRL_ERR_UNSUPPORTED; }
    return SRL_OK;
}

// srl_image_prep.hip: the body of srl_image_prepare / srl_image_prepare_resized behind their upload, on a packed BGR frame of src_rows x
// src_cols that lies on the device (the uploaded one, or srl_jpeg.hip's decoded one): the resize into raw.d unless the frame has the
// preparer's size, then the chain, the hand-over to the colour map and the wait.  The arguments have been checked by the caller.
int srl_prep_run_device(srl_ctx *ctx, const unsigned char *d_bgr, int src_rows, int src_cols, srl_image_prep_info *info);

// srl_color_render.hip: d_bgr (rows x cols x 3, packed, device) becomes the colour map's image as srl_color_image_upload would leave it
int srl_color_image_install(srl_ctx *ctx, const unsigned char *d_bgr, int rows, int cols);
