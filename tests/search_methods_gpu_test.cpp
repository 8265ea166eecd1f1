// The two matchers of GyroAidedTracker (reference include/gyro_aided_tracker.h:132-141) through the API shell on the GPU:
//   SearchByGyroPredict() on a GYRO_PREDICT tracker: mvMatches, mvvNearNeighbors, mvFlowsErrorUn; MatchFeatures() on the
//   lists it left must give the same matches; FindAndSortNearNeighbor() level 1 then 2 on cleared lists must give the same
//   lists; a type-0 tracker answers -1.
//   SearchByOpencvKLT(): mvMatches, mvDisparities, mvPtPredict, mvStatus, mvError.
// Everything is written to <out.bin> for the caller to compare with the C ABI's results.
//   usage: search_methods_gpu_test <in.bin> <out.bin>
//   in : int32 W H N M | u8 ref[W*H] | u8 cur[W*H] | f32 keys_ref[N*2] | f32 keys_cur[M*2] | f32 keys_cur_un[M*2]
//        | f32 fx fy cx cy | f32 dist[4] | f32 gyro[3] | f32 dt
//   out: int32 k | (int32 q, int32 t, f32 dist, f32 ncc)[k] | f32 flows[N*2] | f32 pred_un[N*2] | u8 status[N] | f32 affine[N*4]
//        | int32 lists | int32 k2 | (int32 q, int32 t, f32 dist)[k2] | f64 disp[k2] | f32 pt_predict[N*2] | u8 status[N] | f32 err[N]
#include <cstdio>
#include <cstring>
#include <vector>

#include "gyro_aided_tracker.h"
#include "patch_match.h"

template <class T>
static bool rd(FILE *f, T *p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
template <class T>
static void wr(FILE *f, const T *p, size_t n) { fwrite(p, sizeof(T), n, f); }

static bool same(const GyroAidedTracker::sMatch &a, const GyroAidedTracker::sMatch &b)
{
    return a.queryIdx == b.queryIdx && a.trainIdx == b.trainIdx && !memcmp(&a.distance, &b.distance, 4) && !memcmp(&a.ncc, &b.ncc, 4) &&
           a.level == b.level;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *fi = fopen(argv[1], "rb");
    if (!fi) return 3;
    int hdr[4];
    if (!rd(fi, hdr, 4)) return 4;
    const int W = hdr[0], H = hdr[1], N = hdr[2], M = hdr[3];
    std::vector<unsigned char> ref_px((size_t)W * H), cur_px((size_t)W * H);
    std::vector<float> keys((size_t)N * 2), kc((size_t)M * 2), kcu((size_t)M * 2);
    float kk[4], dc[4], gyro[3], dt;
    if (!rd(fi, ref_px.data(), ref_px.size()) || !rd(fi, cur_px.data(), cur_px.size()) || !rd(fi, keys.data(), keys.size()) ||
        !rd(fi, kc.data(), kc.size()) || !rd(fi, kcu.data(), kcu.size()) || !rd(fi, kk, 4) || !rd(fi, dc, 4) || !rd(fi, gyro, 3) ||
        !rd(fi, &dt, 1))
        return 5;
    fclose(fi);
    cv::Mat K = cv::Mat::eye(3, 3, cv::CV_32F), D(1, 4, cv::CV_32F);
    K.at<float>(0, 0) = kk[0], K.at<float>(1, 1) = kk[1], K.at<float>(0, 2) = kk[2], K.at<float>(1, 2) = kk[3];
    for (int k = 0; k < 4; k++) D.at<float>(k) = dc[k];
    cv::Mat ref(H, W, cv::CV_8UC1, ref_px.data()), cur(H, W, cv::CV_8UC1, cur_px.data());
    std::vector<cv::KeyPoint> kp, kpc, kpcu;
    for (int i = 0; i < N; i++) kp.push_back(cv::KeyPoint(keys[2 * i], keys[2 * i + 1]));
    for (int j = 0; j < M; j++) kpc.push_back(cv::KeyPoint(kc[2 * j], kc[2 * j + 1])), kpcu.push_back(cv::KeyPoint(kcu[2 * j], kcu[2 * j + 1]));
    std::vector<IMU::Point> imu;
    for (int k = 0; k <= 10; k++) imu.push_back(IMU::Point(0, 0, 9.8f, gyro[0], gyro[1], gyro[2], 1.0 + dt * k / 10.0));
    cv::Mat table;
    const cv::Point3f bias(0.f, 0.f, 0.f);
    const int h = 5;
    FILE *fo = fopen(argv[2], "wb");
    if (!fo) return 6;

    // ---- SearchByGyroPredict ----
    GyroAidedTracker T(1.0 + dt, 1.0, ref, cur, kp, kpc, kp, kpcu, imu, bias, K, D, table, GyroAidedTracker::GYRO_PREDICT,
                       GyroAidedTracker::PIXEL_AWARE_PREDICTION, "", h);
    if (!T.mbNCC || T.mRadiusForFindNearNeighbor != 2.0f * h) return 10;
    const int k = T.SearchByGyroPredict();
    if (k < 0 || k != (int)T.mvMatches.size() || (int)T.mvFlowsErrorUn.size() != N || (int)T.mvvNearNeighbors.size() != N) return 11;
    std::vector<GyroAidedTracker::sMatch> again;
    T.MatchFeatures(again, T.mvvNearNeighbors);                      // the public method on the lists that were left
    if (again.size() != T.mvMatches.size()) return 12;
    for (size_t r = 0; r < again.size(); r++)
        if (!same(again[r], T.mvMatches[r])) return 13;
    const std::vector<std::vector<GyroAidedTracker::sMatch>> lists = T.mvvNearNeighbors;
    T.mvvNearNeighbors.assign(N, std::vector<GyroAidedTracker::sMatch>());
    T.FindAndSortNearNeighbor(cv::Range(0, N), 1);                   // the public method, both radii as :912-925 call it
    if (k < 100) T.FindAndSortNearNeighbor(cv::Range(0, N), 2);
    int n_lists = 0;
    for (int i = 0; i < N; i++) {
        if (lists[i].size() != T.mvvNearNeighbors[i].size()) return 14;
        n_lists += !lists[i].empty();
        for (size_t c = 0; c < lists[i].size(); c++)
            if (!same(lists[i][c], T.mvvNearNeighbors[i][c])) return 15;
    }
    wr(fo, &k, 1);
    for (const auto &m : T.mvMatches) wr(fo, &m.queryIdx, 1), wr(fo, &m.trainIdx, 1), wr(fo, &m.distance, 1), wr(fo, &m.ncc, 1);
    wr(fo, reinterpret_cast<const float *>(T.mvFlowsErrorUn.data()), (size_t)N * 2);
    wr(fo, reinterpret_cast<const float *>(T.mvPtPredictUn.data()), (size_t)N * 2);
    wr(fo, T.mvStatus.data(), (size_t)N);
    for (int i = 0; i < N; i++) {
        const cv::Mat &A = T.mvAffineDeformationMatrix[i];
        const float a[4] = {A.empty() ? 1.f : A.at<float>(0, 0), A.empty() ? 0.f : A.at<float>(0, 1), A.empty() ? 0.f : A.at<float>(1, 0),
                            A.empty() ? 1.f : A.at<float>(1, 1)};
        wr(fo, a, 4);
    }
    wr(fo, &n_lists, 1);
    std::printf("SearchByGyroPredict: %d matches, %d features with neighbours\n", k, n_lists);

    // ---- the reference's type dispatch: type 0 is not a type of this method (:899-902) ----
    GyroAidedTracker T0(1.0 + dt, 1.0, ref, cur, kp, kpc, kp, kpcu, imu, bias, K, D, table, GyroAidedTracker::OPENCV_OPTICAL_FLOW_PYR_LK,
                        GyroAidedTracker::PIXEL_AWARE_PREDICTION, "", h);
    if (T0.SearchByGyroPredict() != -1) return 20;

    // ---- SearchByOpencvKLT ----
    const int k2 = T0.SearchByOpencvKLT();
    if (k2 < 0 || k2 != (int)T0.mvMatches.size() || k2 != (int)T0.mvDisparities.size()) return 21;
    wr(fo, &k2, 1);
    for (const auto &m : T0.mvMatches) wr(fo, &m.queryIdx, 1), wr(fo, &m.trainIdx, 1), wr(fo, &m.distance, 1);
    wr(fo, T0.mvDisparities.data(), (size_t)k2);
    wr(fo, reinterpret_cast<const float *>(T0.mvPtPredict.data()), (size_t)N * 2);
    wr(fo, T0.mvStatus.data(), (size_t)N);
    wr(fo, T0.mvError.data(), (size_t)N);
    fclose(fo);
    std::printf("SearchByOpencvKLT: %d matches\n", k2);
    PatchMatch::ReleaseContext();
    std::printf("both Search methods ok\n");
    return 0;
}
