// flow_ref_reader.cpp -- drives the reference's own LKOpticalFlowKernel::trackImage (src/lkpyramid.cpp, compiled where it lies against
// tests/stub_opencv_lk by tests/flow_reader.py) over a sequence of images and hands back the points, the status, the level count and
// every padded level and derivative.  This file holds no code of the reference: it constructs the class with opticalFlowTracker's
// arguments, calls it, and reads its pyramid vectors (private members, opened for this translation unit alone; the layout is unchanged).
#define private public
#include "lkpyramid.h"
#undef private

#include <cstring>
#include <vector>

extern "C" {
void *frr_create(int win, int max_level, int max_count, double epsilon, double min_eig_threshold) {
    cv::TermCriteria criteria(cv::TermCriteria::COUNT + cv::TermCriteria::EPS, max_count, epsilon);
    return new LKOpticalFlowKernel(cv::Size(win, win), max_level, criteria, cv_OPTFLOW_LK_GET_MIN_EIGENVALS, min_eig_threshold);
}
void frr_destroy(void *h) { delete (LKOpticalFlowKernel *)h; }
int frr_max_level(void *h) { return ((LKOpticalFlowKernel *)h)->getMaxLevel(); }
void frr_criteria(void *h, int *max_count, double *epsilon) {
    const cv::TermCriteria c = ((LKOpticalFlowKernel *)h)->getTermCriteria();
    *max_count = c.maxCount; *epsilon = c.epsilon;
}
// gray: rows x cols packed bytes.  status must hold n bytes; it is written only when the class wrote its vector.
int frr_track(void *h, const unsigned char *gray, int rows, int cols, const float *prev_xy, int n, float *next_xy, unsigned char *status) {
    LKOpticalFlowKernel *k = (LKOpticalFlowKernel *)h;
    std::vector<unsigned char> copy(gray, gray + (size_t)rows * cols);
    cv::Mat img(rows, cols, CV_8U, copy.data());
    std::vector<cv::Point2f> last((size_t)n), cur;
    for (int i = 0; i < n; i++) last[i] = cv::Point2f(prev_xy[2 * i], prev_xy[2 * i + 1]);
    std::vector<uchar> st;
    const int got = k->trackImage(img, last, cur, st, 2);
    for (int i = 0; i < n && i < (int)cur.size(); i++) { next_xy[2 * i] = cur[i].x; next_xy[2 * i + 1] = cur[i].y; }
    if ((int)st.size() == n && n) std::memcpy(status, st.data(), (size_t)n);
    return got;
}
// one level of the set the last call's swap left as the PREVIOUS one (the image given last): padded image and padded derivative
int frr_level(void *h, int level, unsigned char *image_padded, short *deriv_padded, int *rows, int *cols) {
    LKOpticalFlowKernel *k = (LKOpticalFlowKernel *)h;
    if (level < 0 || level >= (int)k->prev_img_pyr.size() || level >= (int)k->prev_img_deriv_I_buff.size()) return -1;
    cv::Mat img = k->prev_img_pyr[level];
    *rows = img.rows; *cols = img.cols;
    const int w = k->lk_win_size.width, hh = k->lk_win_size.height;
    img.adjustROI(hh, hh, w, w);
    const cv::Mat &der = k->prev_img_deriv_I_buff[level];
    if (img.rows != *rows + 2 * hh || img.cols != *cols + 2 * w || der.rows != img.rows || der.cols != img.cols) return -2;
    for (int y = 0; y < img.rows; y++) {
        std::memcpy(image_padded + (size_t)y * img.cols, img.ptr(y), (size_t)img.cols);
        std::memcpy(deriv_padded + (size_t)y * der.cols * 2, der.ptr(y), (size_t)der.cols * 2 * sizeof(short));
    }
    return 0;
}
}
