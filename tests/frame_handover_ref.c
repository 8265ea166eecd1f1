/* frame_handover_ref.c -- plain-C restatement of what lies between two frame pairs of the reference's loop:
 *   fhr_post_filter   GyroAidedTracker::GyroPredictFeaturesAndOpticalFlowRefined, Step 3
 *                     (reference src/gyro_aided_tracker.cpp:289-341)
 *   fhr_handover      GyroAidedTracker::SetBackToFrame (:97-111), Frame::SetPredictKeyPointsAndMask
 *                     (reference src/frame.cpp:115-153) and the top-up of Frame::DetectKeyPoints /
 *                     Frame::LoadDetectedKeypointFromFile (:156-218, :244-281), with a full-image mask built exactly as
 *                     the reference builds it (cv::Mat::ones, then a 14 x 14 zero block copied per surviving track)
 *   fhr_predict_live  the outcome include/pagk.h documents for a dead slot of pagk_gyro_predict_device_live
 * Sequential loops in the reference's order.  Shares no code with the kernels (csrc/pagk_handover_kernel.h).
 * Build: gcc -std=c99 -O2 -ffp-contract=off (one rounding per operation). */
#include <stdint.h>
#include <string.h>

/* the camera fields of pagk_params the hand-over reads */
typedef struct fhr_camera {
    float fx, fy, cx, cy;
    float dist_coef[5];
    int32_t n_dist_coef;
} fhr_camera;

/* src/gyro_aided_tracker.cpp:289-341.  thresholds (2 doubles) may be NULL.  Returns the number of survivors. */
int32_t fhr_post_filter(int32_t n, int32_t half_patch, const uint8_t *status_pm, const double *pix_err,
                        const double *dist_pred, const float *pt_pm, const float *pt_pm_un, uint8_t *status_out,
                        float *pt_predict, float *pt_predict_un, double *thresholds)
{
    double sum = 0.0; /* :296 */
    int cnt = 0;
    int32_t i, kept = 0;
    double avg, th_pix, th_dist;
    for (i = 0; i < n; i++) { /* :297 */
        if (status_pm[i]) {   /* :298 */
            sum += pix_err[i]; /* :299 */
            cnt++;             /* :300 */
        }
    }
    avg = sum / cnt;                                                    /* :305: 0 / 0 = NaN when nothing was tracked   */
    th_pix = 4.0 * avg > half_patch ? 4.0 * avg : (double)half_patch;   /* :308 std::max(4 * avg, (double)h): NaN -> h   */
    th_dist = half_patch * 4.0;                                         /* :312                                          */
    for (i = 0; i < n; i++) {                                           /* :318                                          */
        if (status_pm[i] && pix_err[i] < th_pix && dist_pred[i] < th_dist) { /* :319-321 */
            status_out[i] = 1;                                          /* :322 */
            if (pt_predict && pt_pm) {                                  /* :323 */
                pt_predict[2 * i] = pt_pm[2 * i];
                pt_predict[2 * i + 1] = pt_pm[2 * i + 1];
            }
            if (pt_predict_un && pt_pm_un) {                            /* :324 */
                pt_predict_un[2 * i] = pt_pm_un[2 * i];
                pt_predict_un[2 * i + 1] = pt_pm_un[2 * i + 1];
            }
            kept++;
        } else {
            status_out[i] = 0;                                          /* :327 */
        }
    }
    if (thresholds) {
        thresholds[0] = th_pix;
        thresholds[1] = th_dist;
    }
    return kept;
}

/* src/frame.cpp:148-149 for one axis */
static int fhr_origin(float v, int extent)
{
    const int half_path_size = 7;                /* :117 */
    int a = (int)v - half_path_size;             /* int(pt_pred_un.x) - half_path_size */
    if (a < 0) a = 0;                            /* std::max(0, .) */
    if (a > extent - 2 * half_path_size) a = extent - 2 * half_path_size; /* std::min(., width - roi.cols) */
    return a;
}

/* Exposed for the clamp test: the origin of the hole of a track at (x_un, y_un). */
void fhr_hole_origin(float x_un, float y_un, int32_t width, int32_t height, int32_t *x0, int32_t *y0)
{
    *x0 = fhr_origin(x_un, width);
    *y0 = fhr_origin(y_un, height);
}

/* DistortVecPoints, src/utils.cpp:49-76, one point; a copy when k1 == 0 (src/patch_match.cpp:410-411) */
static void fhr_distort(const fhr_camera *c, float px, float py, float *ox, float *oy)
{
    float mfx_inv = (float)(1.0 / c->fx), mfy_inv = (float)(1.0 / c->fy); /* :53 */
    float K1 = c->dist_coef[0], K2 = c->dist_coef[1], mp1 = c->dist_coef[2], mp2 = c->dist_coef[3];
    float K3 = c->n_dist_coef == 5 ? c->dist_coef[4] : 0.0f;              /* :57 */
    float x, y, r2, r4, r6, x_distort, y_distort;
    if (K1 == 0.0f) {
        *ox = px;
        *oy = py;
        return;
    }
    x = (px - c->cx) * mfx_inv; /* :63 */
    y = (py - c->cy) * mfy_inv; /* :64 */
    r2 = x * x + y * y;         /* :66 */
    r4 = r2 * r2;
    r6 = r4 * r2;
    x_distort = x * (1 + K1 * r2 + K2 * r4 + K3 * r6) + 2 * mp1 * x * y + mp2 * (r2 + 2 * x * x); /* :69 */
    y_distort = y * (1 + K1 * r2 + K2 * r4 + K3 * r6) + mp1 * (r2 + 2 * y * y) + 2 * mp2 * x * y; /* :70 */
    *ox = c->fx * x_distort + c->cx; /* :71 */
    *oy = c->fy * y_distort + c->cy; /* :72 */
}

/* The hand-over.  status / pt_predict / pt_predict_un: cap entries; cand_un: n_cand points; outputs: cap entries each,
 * mask width * height bytes, state 8 words ([1] = reach_max_feature_flag, read and written). */
void fhr_handover(const fhr_camera *cam, int32_t width, int32_t height, int32_t cap, int32_t target_n,
                  double new_point_threshold, const uint8_t *status, const float *pt_predict, const float *pt_predict_un,
                  int32_t n_cand, const float *cand_un, float *keys, float *keys_un, float *keys_normal,
                  int32_t *index_in_last, uint8_t *live, uint8_t *mask, int32_t *state)
{
    const int half_path_size = 7;                                           /* src/frame.cpp:117 */
    const float mfx_inv = (float)(1.0 / cam->fx), mfy_inv = (float)(1.0 / cam->fy); /* :70 */
    int32_t size = 0; /* mvKeysUn.size() */
    int32_t i, j, r, c, num_predicted, rejected = 0, added = 0, reach = state[1];
    memset(mask, 1, (size_t)width * height);                                /* :89 cv::Mat::ones */
    for (i = 0; i < cap; i++) {                                             /* :120 */
        float xu, yu;
        int _x, _y;
        if (!status[i]) continue;                                           /* :122 */
        xu = pt_predict_un[2 * i], yu = pt_predict_un[2 * i + 1];           /* :126 */
        keys[2 * size] = pt_predict[2 * i], keys[2 * size + 1] = pt_predict[2 * i + 1]; /* :132 */
        keys_un[2 * size] = xu, keys_un[2 * size + 1] = yu;                 /* :133 */
        if (keys_normal) {
            keys_normal[2 * size] = (xu - cam->cx) * mfx_inv;               /* :128 */
            keys_normal[2 * size + 1] = (yu - cam->cy) * mfy_inv;           /* :129 */
        }
        index_in_last[size] = i;                                            /* :135 */
        size++;
        _x = fhr_origin(xu, width);                                         /* :148 */
        _y = fhr_origin(yu, height);                                        /* :149 */
        for (r = 0; r < 2 * half_path_size; r++)                            /* :150-151 roi.copyTo(mMask(roi_rect)) */
            for (c = 0; c < 2 * half_path_size; c++) mask[(size_t)(_y + r) * width + _x + c] = 0;
    }
    num_predicted = size;                                                   /* :159 / :245 */
    /* the acceptance test over the whole list (state[4]); accepted candidates do not change the mask (:252-266) */
    for (j = 0; j < n_cand; j++) {
        float x = cand_un[2 * j], y = cand_un[2 * j + 1];
        int inside = x > -1.0f && x < (float)width && y > -1.0f && y < (float)height; /* int() lands in the image */
        if (!inside || mask[(size_t)(int)y * width + (int)x] == 0) rejected++;       /* :253 */
    }
    if (num_predicted < new_point_threshold || !reach) {                    /* :164 */
        int32_t n_new = target_n - num_predicted;                           /* :168 */
        if (n_new > 0) {                                                    /* :169 (the early return keeps the flag) */
            for (j = 0; j < n_cand; j++) {                                  /* :252 */
                float x = cand_un[2 * j], y = cand_un[2 * j + 1], dx, dy;
                int inside = x > -1.0f && x < (float)width && y > -1.0f && y < (float)height;
                if (!inside || mask[(size_t)(int)y * width + (int)x] == 0) continue; /* :253-254 */
                keys_un[2 * size] = x, keys_un[2 * size + 1] = y;           /* :257 */
                index_in_last[size] = -1;                                   /* :258 */
                if (keys_normal) {
                    keys_normal[2 * size] = (x - cam->cx) * mfx_inv;        /* :259 */
                    keys_normal[2 * size + 1] = (y - cam->cy) * mfy_inv;    /* :260 */
                }
                fhr_distort(cam, x, y, &dx, &dy);                           /* :270-273 */
                keys[2 * size] = dx, keys[2 * size + 1] = dy;
                size++;
                added++;
                n_new--;                                                    /* :263 */
                if (n_new <= 0) break;                                      /* :264 */
            }
            reach = size == target_n;                                       /* :214 */
        }
    }
    for (i = 0; i < cap; i++) {
        live[i] = i < size;
        if (i >= size) {
            keys[2 * i] = keys[2 * i + 1] = 0.0f;
            keys_un[2 * i] = keys_un[2 * i + 1] = 0.0f;
            if (keys_normal) keys_normal[2 * i] = keys_normal[2 * i + 1] = 0.0f;
            index_in_last[i] = -1;
        }
    }
    state[0] = size; /* :217 mN = mvKeysUn.size() */
    state[1] = reach;
    state[2] = num_predicted;
    state[3] = added;
    state[4] = rejected;
    state[5] = state[6] = state[7] = 0;
}

/* A dead slot after pagk_gyro_predict_device_live: the tracker's initial state (src/gyro_aided_tracker.cpp:92-95,
 * :131-135), affine untouched.  Applied on top of the arrays a full prediction wrote. */
void fhr_predict_live(int32_t n, const uint8_t *live, float *pt_predict_un, float *pt_predict, uint8_t *status)
{
    int32_t i;
    for (i = 0; i < n; i++)
        if (!live[i]) {
            status[i] = 0;
            pt_predict_un[2 * i] = pt_predict_un[2 * i + 1] = 0.0f;
            pt_predict[2 * i] = pt_predict[2 * i + 1] = 0.0f;
        }
}
