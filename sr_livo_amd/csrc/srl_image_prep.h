// srl_image_prep.h -- internal: the image preparer's state (srl_image_prep.hip), read by srl_flow.hip (srl_flow_track_prepared takes
// d_gray_eq as its image).  Every plane is allocated for the pixel count rounded up to a multiple of 4: the per-pixel kernels load and
// store four pixels per lane, the last lane's surplus lands in that slack and is never downloaded.
#pragma once
#include "srl_ctx.h"

struct SrlImagePrep {
    srl_image_prep_opts opts;
    int rows = 0, cols = 0;
    int T = 0, tw = 0, th = 0, ext_rows = 0, ext_cols = 0;      // tiles per side, tile size, the (possibly) extended plane
    int limit[2] = {0, 0};                                      // clip limit of a tile's bins: [0] gray, [1] Y
    bool have_image = false;
    unsigned char *h_raw = nullptr;                             // page-locked staging of the upload, rows packed
    unsigned char *d_raw = nullptr;                             // rows x cols x 3
    short *d_map1 = nullptr;                                    // (sx, sy) per pixel
    unsigned short *d_map2 = nullptr;                           // ay * 32 + ax per pixel
    unsigned char *d_undist = nullptr, *d_gray = nullptr, *d_y = nullptr, *d_crcb = nullptr;      // 3, 1, 1, 2 bytes per pixel
    unsigned char *d_lut = nullptr;                             // [plane][ty][tx][256]: plane 0 gray, 1 Y
    unsigned char *d_gray_eq = nullptr, *d_bgr_eq = nullptr;    // the two results
};

// srl_color_render.hip: d_bgr (rows x cols x 3, packed, device) becomes the colour map's image as srl_color_image_upload would leave it
int srl_color_image_install(srl_ctx *ctx, const unsigned char *d_bgr, int rows, int cols);
