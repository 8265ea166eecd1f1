// gyro_aided_tracker.cpp -- host side of the hot path: producer of PatchMatch's inputs and consumer
// of its outputs, with the reference's names and arithmetic (src/gyro_aided_tracker.cpp:11-95,118-426,
// 511-587).  float32 throughout, double where the reference's expressions promote.
#include "gyro_aided_tracker.h"

#include <chrono>
#include <cmath>
#include <stdexcept>

#include "pagk.h"
#include "patch_match.h"

// reference src/gyro_aided_tracker.cpp:11-28.  NB: like the reference, mvKeysRefUn binds to
// vKeysRef_ (not vKeysUnRef_), :21.
GyroAidedTracker::GyroAidedTracker(double t, double t_ref, const cv::Mat &imgGrayRef_, const cv::Mat &imgGrayCur_,
                                   const std::vector<cv::KeyPoint> &vKeysRef_,
                                   const std::vector<cv::KeyPoint> &vKeysCur_,
                                   const std::vector<cv::KeyPoint> &vKeysUnRef_,
                                   const std::vector<cv::KeyPoint> &vKeysUnCur_,
                                   const std::vector<IMU::Point> &vImuFromLastFrame, const cv::Point3f &bias_,
                                   cv::Mat K_, cv::Mat DistCoef_, const cv::Mat &normalizeTable_, eType type_,
                                   ePredictMethod predictMethod_, std::string saveFolderPath, int halfPatchSize_)
    : mTimeStamp(t), mTimeStampRef(t_ref), mImgGrayRef(imgGrayRef_), mImgGrayCur(imgGrayCur_), mvKeysRef(vKeysRef_),
      mvKeysRefUn(vKeysRef_), mvKeysCur(vKeysCur_), mvKeysCurUn(vKeysUnCur_), mvImuFromLastFrame(vImuFromLastFrame),
      mHalfPatchSize(halfPatchSize_), mBias(bias_), mK(K_), mDistCoef(DistCoef_), mWidth(imgGrayCur_.cols),
      mHeight(imgGrayCur_.rows), mNormalizeTable(normalizeTable_), mType(type_), mPredictMethod(predictMethod_)
{
    (void)vKeysUnRef_;
    (void)saveFolderPath;  // result logging is out of scope
    mRbc = cv::Mat::eye(3, 3, cv::CV_32F);
    Initialize();
}

// reference :51-95
void GyroAidedTracker::Initialize()
{
    mHalfPatchSize = mHalfPatchSize == 0 ? 5 : mHalfPatchSize;  // :61
    mfx = mK.at<float>(0, 0), mfy = mK.at<float>(1, 1);
    mcx = mK.at<float>(0, 2), mcy = mK.at<float>(1, 2);
    mfx_inv = (float)(1.0 / mfx), mfy_inv = (float)(1.0 / mfy);  // :66
    mk1 = mDistCoef.at<float>(0), mk2 = mDistCoef.at<float>(1);
    mp1 = mDistCoef.at<float>(2), mp2 = mDistCoef.at<float>(3);
    mk3 = mDistCoef.total() == 5 ? mDistCoef.at<float>(4) : 0;
    mvPatchCorners.resize(4);
    const float h = (float)mHalfPatchSize;
    mvPatchCorners[0] = cv::Point2f(-h, -h);  // top left      :73-77
    mvPatchCorners[1] = cv::Point2f(h, -h);   // top right
    mvPatchCorners[2] = cv::Point2f(-h, h);   // bottom left
    mvPatchCorners[3] = cv::Point2f(h, h);    // bottom right
    mbNCC = true;                                              // :60
    mRadiusForFindNearNeighbor = 2.0f * (float)mHalfPatchSize;  // :62
    mN = (int)mvKeysRef.size();
    mvvNearNeighbors.assign(mvKeysRef.size(), std::vector<sMatch>());
    mvFlowsErrorUn.assign(mvKeysRef.size(), cv::Point2f(0, 0));
    mvPtPredict.assign(mN, cv::Point2f(0, 0));
    mvPtPredictUn.assign(mN, cv::Point2f(0, 0));
    mvFlowsPredictUn.assign(mN, cv::Point2f(0, 0));
    mvStatus.assign(mN, 0);
    mvError.resize(mN);
    mvvPtPredictCorners.resize(mN);
    mvvPtPredictCornersUn.resize(mN);
    mvvFlowsPredictCorners.resize(mN);
    mvAffineDeformationMatrix.assign(mN, cv::Mat());
}

static cv::Mat inv3(const cv::Mat &m)
{
    double a[3][3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) a[r][c] = m.at<float>(r, c);
    double det = a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
                 a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
    cv::Mat o(3, 3, cv::CV_32F);
    double d = det != 0 ? 1.0 / det : 0;
    o.at<float>(0, 0) = (float)((a[1][1] * a[2][2] - a[1][2] * a[2][1]) * d);
    o.at<float>(0, 1) = (float)((a[0][2] * a[2][1] - a[0][1] * a[2][2]) * d);
    o.at<float>(0, 2) = (float)((a[0][1] * a[1][2] - a[0][2] * a[1][1]) * d);
    o.at<float>(1, 0) = (float)((a[1][2] * a[2][0] - a[1][0] * a[2][2]) * d);
    o.at<float>(1, 1) = (float)((a[0][0] * a[2][2] - a[0][2] * a[2][0]) * d);
    o.at<float>(1, 2) = (float)((a[0][2] * a[1][0] - a[0][0] * a[1][2]) * d);
    o.at<float>(2, 0) = (float)((a[1][0] * a[2][1] - a[1][1] * a[2][0]) * d);
    o.at<float>(2, 1) = (float)((a[0][1] * a[2][0] - a[0][0] * a[2][1]) * d);
    o.at<float>(2, 2) = (float)((a[0][0] * a[1][1] - a[0][1] * a[1][0]) * d);
    return o;
}

// reference :511-519
void GyroAidedTracker::SetRcl(const cv::Mat Rcl_)
{
    mRcl = Rcl_.clone();
    mr11 = mRcl.at<float>(0, 0), mr12 = mRcl.at<float>(0, 1), mr13 = mRcl.at<float>(0, 2);
    mr21 = mRcl.at<float>(1, 0), mr22 = mRcl.at<float>(1, 1), mr23 = mRcl.at<float>(1, 2);
    mr31 = mRcl.at<float>(2, 0), mr32 = mRcl.at<float>(2, 1), mr33 = mRcl.at<float>(2, 2);
    mKRKinv = mK * mRcl * inv3(mK);
}

// reference :521-562
void GyroAidedTracker::IntegrateGyroMeasurements()
{
    cv::Mat dR = cv::Mat::eye(3, 3, cv::CV_32F);
    const int n = (int)mvImuFromLastFrame.size() - 1;
    for (int i = 0; i < n; i++) {
        float tstep = 0;
        cv::Point3f angVel;
        const IMU::Point &p0 = mvImuFromLastFrame[i], &p1 = mvImuFromLastFrame[i + 1];
        if ((i == 0) && (i < (n - 1))) {
            float tab = (float)(p1.t - p0.t);
            float tini = (float)(p0.t - mTimeStampRef);
            angVel = (p0.w + p1.w - (p1.w - p0.w) * (tini / tab)) * 0.5f;
            tstep = (float)(p1.t - mTimeStampRef);
        } else if (i < (n - 1)) {
            angVel = (p0.w + p1.w) * 0.5f;
            tstep = (float)(p1.t - p0.t);
        } else if ((i > 0) && (i == (n - 1))) {
            float tab = (float)(p1.t - p0.t);
            float tend = (float)(p1.t - mTimeStamp);
            angVel = (p0.w + p1.w - (p1.w - p0.w) * (tend / tab)) * 0.5f;
            tstep = (float)(mTimeStamp - p0.t);
        } else if ((i == 0) && (i == (n - 1))) {
            angVel = p0.w;
            tstep = (float)(mTimeStamp - mTimeStampRef);
        }
        dR = dR * IntegrateOneGyroMeasurement(angVel, tstep);
    }
    SetRcl(mRbc.t() * dR.t() * mRbc);  // :560
}

// reference :564-587
cv::Mat GyroAidedTracker::IntegrateOneGyroMeasurement(cv::Point3f &gyro, double dt)
{
    const float x = (float)((gyro.x - mBias.x) * dt);
    const float y = (float)((gyro.y - mBias.y) * dt);
    const float z = (float)((gyro.z - mBias.z) * dt);
    const float d2 = x * x + y * y + z * z;
    const float d = std::sqrt(d2);
    cv::Mat W(3, 3, cv::CV_32F);
    const float w[9] = {0, -z, y, z, 0, -x, -y, x, 0};
    for (int k = 0; k < 9; k++) W.at<float>(k / 3, k % 3) = w[k];
    cv::Mat R = cv::Mat::eye(3, 3, cv::CV_32F);
    if (d < 1e-4) {
        for (int k = 0; k < 9; k++) R.at<float>(k / 3, k % 3) += w[k];
    } else {
        cv::Mat WW = W * W;
        const double s = std::sin(d), c = 1.0f - std::cos(d);
        for (int k = 0; k < 9; k++)
            R.at<float>(k / 3, k % 3) =
                (float)((double)R.at<float>(k / 3, k % 3) + (double)w[k] * s / d + (double)WW.at<float>(k / 3, k % 3) * c / d2);
    }
    return R;
}

// reference :194-231 (PIXEL_AWARE_PREDICTION) and :233-253 (SINGLE_HOMOGRAPHY: lambda = 1)
void GyroAidedTracker::GyroPredictOnePixel(cv::Point2f &pt_ref, cv::Point2f &pt_predict,
                                           cv::Point2f &pt_predict_distort, cv::Point2f &flow)
{
    float x_normal = (pt_ref.x - mcx) * mfx_inv;
    float y_normal = (pt_ref.y - mcy) * mfy_inv;
    float lambda = mPredictMethod == PIXEL_AWARE_PREDICTION
                       ? (float)(1.0 / (mr31 * x_normal + mr32 * y_normal + mr33))
                       : 1.0f;
    float pt_x = (mKRKinv.at<float>(0, 0) * pt_ref.x + mKRKinv.at<float>(0, 1) * pt_ref.y + mKRKinv.at<float>(0, 2)) * lambda;
    float pt_y = (mKRKinv.at<float>(1, 0) * pt_ref.x + mKRKinv.at<float>(1, 1) * pt_ref.y + mKRKinv.at<float>(1, 2)) * lambda;
    pt_predict = cv::Point2f(pt_x, pt_y);
    float x = (pt_predict.x - mcx) * mfx_inv;
    float y = (pt_predict.y - mcy) * mfy_inv;
    float r2 = x * x + y * y;
    float r4 = r2 * r2;
    float r6 = r4 * r2;
    float x_distort = x * (1 + mk1 * r2 + mk2 * r4 + mk3 * r6) + 2 * mp1 * x * y + mp2 * (r2 + 2 * x * x);
    float y_distort = y * (1 + mk1 * r2 + mk2 * r4 + mk3 * r6) + mp1 * (r2 + 2 * y * y) + 2 * mp2 * x * y;
    pt_predict_distort = cv::Point2f(mfx * x_distort + mcx, mfy * y_distort + mcy);
    flow = pt_predict - pt_ref;
}

// reference :118-185
int GyroAidedTracker::GyroPredictFeatures()
{
    auto t1 = std::chrono::steady_clock::now();
    const float hh = (float)mHalfPatchSize;
    // (B B^T)^-1 for B = [+-h corner matrix]: diag(1/(4h^2)) through the double determinant (cv::Mat::inv, 2x2)
    const float m00 = 4 * hh * hh;
    const double det = (double)m00 * m00;
    const double dinv = det != 0 ? 1. / det : 0;
    const float inv00 = (float)(m00 * dinv), inv01 = (float)(-0.0f * dinv);
    for (int i = 0; i < mN; i++) {
        cv::Point2f pt_ref_un = mvKeysRefUn[i].pt, pu, pd, flow;
        GyroPredictOnePixel(pt_ref_un, pu, pd, flow);
        if (pu.x < 0 || pu.x >= mWidth || pu.y < 0 || pu.y >= mHeight) continue;  // :131
        if (pd.x < 0 || pd.x >= mWidth || pd.y < 0 || pd.y >= mHeight) continue;  // :134
        mvPtPredictUn[i] = pu;
        mvPtPredict[i] = pd;
        mvStatus[i] = true;
        mvFlowsPredictUn[i] = flow;
        std::vector<cv::Point2f> corners, cornersUn, vecC;
        for (size_t j = 0; j < mvPatchCorners.size(); j++) {  // :148-160
            cv::Point2f c_un(mvKeysRefUn[i].pt + mvPatchCorners[j]), cu, cd, cf;
            GyroPredictOnePixel(c_un, cu, cd, cf);
            cornersUn.push_back(cu);
            corners.push_back(cd);
            vecC.push_back(cu - pu);
        }
        mvvPtPredictCorners[i] = corners;
        mvvPtPredictCornersUn[i] = cornersUn;
        mvvFlowsPredictCorners[i] = vecC;
        // A = C * B^T * (B * B^T)^-1, :166-167 (float products, double accumulation per Mat product)
        double s00 = 0, s01 = 0, s10 = 0, s11 = 0;
        for (int j = 0; j < 4; j++) {
            s00 += (double)vecC[j].x * mvPatchCorners[j].x;
            s01 += (double)vecC[j].x * mvPatchCorners[j].y;
            s10 += (double)vecC[j].y * mvPatchCorners[j].x;
            s11 += (double)vecC[j].y * mvPatchCorners[j].y;
        }
        const float t00 = (float)s00, t01 = (float)s01, t10 = (float)s10, t11 = (float)s11;
        cv::Mat A(2, 2, cv::CV_32F);
        A.at<float>(0, 0) = (float)((double)t00 * inv00 + (double)t01 * inv01);
        A.at<float>(0, 1) = (float)((double)t00 * inv01 + (double)t01 * inv00);
        A.at<float>(1, 0) = (float)((double)t10 * inv00 + (double)t11 * inv01);
        A.at<float>(1, 1) = (float)((double)t10 * inv01 + (double)t11 * inv00);
        mvAffineDeformationMatrix[i] = A;
    }
    int n_predict = 0;
    for (auto s : mvStatus) n_predict += s ? 1 : 0;
    mTimeCostGyroPredict = std::chrono::duration<float>(std::chrono::steady_clock::now() - t1).count();
    mvPtGyroPredict = mvPtPredict;
    mvPtGyroPredictUn = mvPtPredictUn;
    return n_predict;
}

// reference :258-342
int GyroAidedTracker::GyroPredictFeaturesAndOpticalFlowRefined()
{
    if (mbHasGyroPredictInitial)
        GyroPredictFeatures();
    else {
        for (int i = 0; i < mN; i++) {  // :264-270
            mvPtPredictUn[i] = mvKeysRefUn[i].pt;
            mvPtPredict[i] = mvKeysRef[i].pt;
            mvStatus[i] = true;
            mvFlowsPredictUn[i] = cv::Point2f(0, 0);
            mvAffineDeformationMatrix[i] = cv::Mat::eye(2, 2, cv::CV_32F);
        }
    }
    auto t1 = std::chrono::steady_clock::now();
    const bool inverse = false;  // :278
    PatchMatch patchMatch(this, mHalfPatchSize, mIterations, mPyramids, mbHasGyroPredictInitial, inverse,
                          mbConsiderIllumination, mbConsiderAffineDeformation, mbRegularizationPenalty);
    patchMatch.OpticalFlowMultiLevel();
    mTimeCostOptFlow = std::chrono::duration<float>(std::chrono::steady_clock::now() - t1).count();

    auto t3 = std::chrono::steady_clock::now();
    // Step 3 (:289-341): thresholds from the mean pixel error, final mask, survivors copied back
    std::vector<cv::uchar> status(mN ? mN : 1);
    int n_predict = pagk_post_filter(mN, mHalfPatchSize, mvStatusAfterPatchMatched.data(),
                                     mvPixelErrorsOfPatchMatched.data(), mvDistanceBetweenPredictedAndPatchMatched.data(),
                                     reinterpret_cast<const float *>(mvPtPredictAfterPatchMatched.data()),
                                     reinterpret_cast<const float *>(mvPtPredictAfterPatchMatchedUn.data()),
                                     status.data(), reinterpret_cast<float *>(mvPtPredict.data()),
                                     reinterpret_cast<float *>(mvPtPredictUn.data()));
    if (n_predict < 0) throw std::runtime_error("pagk_post_filter failed");
    for (int i = 0; i < mN; i++) mvStatus[i] = status[i];
    mTimeCostOptFlowResultFilterOut = std::chrono::duration<float>(std::chrono::steady_clock::now() - t3).count();
    return n_predict;
}

// reference :344-426
int GyroAidedTracker::TrackFeatures()
{
    IntegrateGyroMeasurements();
    int n_predict = -1;
    if (mType == OPENCV_OPTICAL_FLOW_PYR_LK) {
        // :353-380.  cv::calcOpticalFlowPyrLK is the library's pagk_lk_track (its definition, not OpenCV's arithmetic:
        // include/pagk.h "Pyramidal Lucas-Kanade") with the constants of :361-366 and the error filter of :371-375.
        std::vector<float> ptRef(2 * (size_t)mN + 2), ptOut(2 * (size_t)mN + 2, 0.f), flow(2 * (size_t)mN + 2, 0.f);
        std::vector<cv::uchar> status((size_t)mN + 1, 0);
        for (int i = 0; i < mN; i++) ptRef[2 * i] = mvKeysRefUn[i].pt.x, ptRef[2 * i + 1] = mvKeysRefUn[i].pt.y;  // :355-358
        pagk_lk_params lk;
        pagk_lk_params_default(&lk);  // maxLevel 2, (COUNT + EPS, 30, 0.01), minEigThreshold 1e-4, 12.0
        lk.half_patch = mHalfPatchSize;  // :361
        const cv::Mat &r = mImgGrayRef, &c = mImgGrayCur;
        pagk_image ref{r.data, r.cols, r.rows, (int64_t)r.step}, cur{c.data, c.cols, c.rows, (int64_t)c.step};
        mvError.assign(mN, 0.f);
        int32_t info[PAGK_LK_INFO_WORDS] = {0};
        int rc = pagk_lk_track(PatchMatch::Context(), &lk, &ref, &cur, mN, ptRef.data(), ptOut.data(), status.data(), nullptr,
                               mN ? mvError.data() : nullptr, flow.data(), info);
        if (rc != PAGK_OK)
            throw std::runtime_error(std::string("GyroAidedTracker::TrackFeatures: pagk_lk_track: ") + pagk_strerror(rc) + " " +
                                     pagk_last_error(PatchMatch::Context()));
        mvPtPredictUn.resize(mN);
        for (int i = 0; i < mN; i++) {
            mvPtPredictUn[i] = cv::Point2f(ptOut[2 * i], ptOut[2 * i + 1]);
            mvStatus[i] = status[i];                                              // :371-373
            mvFlowsPredictUn[i] = cv::Point2f(flow[2 * i], flow[2 * i + 1]);      // :375
        }
        PatchMatch::DistortVecPoints(mvPtPredictUn, mvPtPredict, mK, mDistCoef);  // :379
        // The reference returns n_predict uninitialised on this branch; the library's rule: the number of kept features.
        n_predict = info[2];
    } else if (mType == GYRO_PREDICT) {
        n_predict = GyroPredictFeatures();
    } else {
        switch (mType) {  // :384-414
            case IMAGE_ONLY_OPTICAL_FLOW_CONSIDER_ILLUMINATION:
                mbHasGyroPredictInitial = false, mbConsiderIllumination = true, mbConsiderAffineDeformation = true,
                mbRegularizationPenalty = false;
                break;
            case GYRO_PREDICT_WITH_OPTICAL_FLOW_REFINED:
                mbHasGyroPredictInitial = true, mbConsiderIllumination = false, mbConsiderAffineDeformation = false,
                mbRegularizationPenalty = false;
                break;
            case GYRO_PREDICT_WITH_OPTICAL_FLOW_REFINED_CONSIDER_ILLUMINATION:
                mbHasGyroPredictInitial = true, mbConsiderIllumination = true, mbConsiderAffineDeformation = false,
                mbRegularizationPenalty = false;
                break;
            case GYRO_PREDICT_WITH_OPTICAL_FLOW_REFINED_CONSIDER_ILLUMINATION_DEFORMATION:
                mbHasGyroPredictInitial = true, mbConsiderIllumination = true, mbConsiderAffineDeformation = true,
                mbRegularizationPenalty = false;
                break;
            case GYRO_PREDICT_WITH_OPTICAL_FLOW_REFINED_CONSIDER_ILLUMINATION_DEFORMATION_REGULAR:
                mbHasGyroPredictInitial = true, mbConsiderIllumination = true, mbConsiderAffineDeformation = true,
                mbRegularizationPenalty = true;
                break;
            default:
                return -1;  // :415-418 "Unsupport type"
        }
        n_predict = GyroPredictFeaturesAndOpticalFlowRefined();
    }
    return n_predict;
}

// ---- track-to-detection association (reference :788-1136; the definition is in include/pagk.h) ---------------------------
namespace {
struct KeyArrays {
    std::vector<float> ref, pred, affine, cur, cur_un;
    std::vector<cv::uchar> status;
};

// the tracker's vectors as the dense arrays of the C ABI (one spare row: no array is empty)
KeyArrays key_arrays(const GyroAidedTracker &t)
{
    const size_t n = (size_t)t.mN, m = t.mvKeysCur.size();
    KeyArrays a;
    a.ref.assign(2 * n + 2, 0.f), a.pred.assign(2 * n + 2, 0.f), a.affine.assign(4 * n + 4, 0.f), a.status.assign(n + 1, 0);
    a.cur.assign(2 * m + 2, 0.f), a.cur_un.assign(2 * m + 2, 0.f);
    for (size_t i = 0; i < n; i++) {
        a.ref[2 * i] = t.mvKeysRef[i].pt.x, a.ref[2 * i + 1] = t.mvKeysRef[i].pt.y;
        a.pred[2 * i] = t.mvPtPredictUn[i].x, a.pred[2 * i + 1] = t.mvPtPredictUn[i].y;
        a.status[i] = t.mvStatus[i];
        const cv::Mat &A = t.mvAffineDeformationMatrix[i];  // an empty Mat warps nothing (src/utils.cpp:125)
        a.affine[4 * i] = A.empty() ? 1.f : A.at<float>(0, 0), a.affine[4 * i + 1] = A.empty() ? 0.f : A.at<float>(0, 1);
        a.affine[4 * i + 2] = A.empty() ? 0.f : A.at<float>(1, 0), a.affine[4 * i + 3] = A.empty() ? 1.f : A.at<float>(1, 1);
    }
    for (size_t j = 0; j < m; j++) {
        a.cur[2 * j] = t.mvKeysCur[j].pt.x, a.cur[2 * j + 1] = t.mvKeysCur[j].pt.y;
        a.cur_un[2 * j] = t.mvKeysCurUn[j].pt.x, a.cur_un[2 * j + 1] = t.mvKeysCurUn[j].pt.y;
    }
    return a;
}

pagk_image image_of(const cv::Mat &m) { return pagk_image{m.data, m.cols, m.rows, (int64_t)m.step}; }

[[noreturn]] void fail(const char *what, int rc)
{
    throw std::runtime_error(std::string("GyroAidedTracker: ") + what + ": " + pagk_strerror(rc) + " " +
                             pagk_last_error(PatchMatch::Context()));
}
}  // namespace

// reference :788-851 for the features of `range`: the lists of features that have none yet
void GyroAidedTracker::FindAndSortNearNeighbor(const cv::Range &range, int level)
{
    const KeyArrays a = key_arrays(*this);
    const int m = (int)mvKeysCur.size();
    std::vector<int32_t> count((size_t)mN + 1, 0);
    for (int i = 0; i < mN; i++)  // a feature outside the range, or with a list (:793), is skipped
        count[i] = (i < range.start || i >= range.end) ? 1 : (int32_t)mvvNearNeighbors[i].size();
    const std::vector<int32_t> before = count;
    const pagk_image ref = image_of(mImgGrayRef), cur = image_of(mImgGrayCur);
    int cap = 64;
    for (;;) {
        std::vector<int32_t> idx((size_t)mN * cap + 1), cnt = before;
        std::vector<float> dist((size_t)mN * cap + 1), ncc((size_t)mN * cap + 1);
        int rc = pagk_find_near_neighbors(PatchMatch::Context(), &ref, &cur, mHalfPatchSize, mN, a.ref.data(), a.pred.data(),
                                          a.status.data(), a.affine.data(), m, a.cur.data(), a.cur_un.data(), level,
                                          mRadiusForFindNearNeighbor, mbNCC ? 1 : 0, cap, cnt.data(), idx.data(), dist.data(),
                                          ncc.data());
        if (rc == PAGK_E_CAPACITY) {  // cnt holds the sizes needed
            for (int i = 0; i < mN; i++) cap = cnt[i] > cap ? cnt[i] : cap;
            continue;
        }
        if (rc != PAGK_OK) fail("pagk_find_near_neighbors", rc);
        for (int i = range.start; i < range.end && i < mN; i++) {
            if (before[i] > 0 || !mvStatus[i]) continue;
            std::vector<sMatch> &list = mvvNearNeighbors[i];
            for (int k = 0; k < cnt[i]; k++)
                list.push_back(sMatch(i, idx[(size_t)i * cap + k], dist[(size_t)i * cap + k], ncc[(size_t)i * cap + k], level));
        }
        return;
    }
}

// reference :949-1008
void GyroAidedTracker::MatchFeatures(std::vector<sMatch> &vMatches, const std::vector<std::vector<sMatch>> &vvNearNeighbors)
{
    size_t cap = 1;
    for (int i = 0; i < mN; i++) cap = vvNearNeighbors[i].size() > cap ? vvNearNeighbors[i].size() : cap;
    std::vector<int32_t> count((size_t)mN + 1, 0), idx((size_t)mN * cap + 1, -1), q((size_t)mN + 1), t((size_t)mN + 1);
    std::vector<float> dist((size_t)mN * cap + 1, 0.f), ncc((size_t)mN * cap + 1, 0.f), md((size_t)mN + 1), mc((size_t)mN + 1);
    for (int i = 0; i < mN; i++) {
        count[i] = (int32_t)vvNearNeighbors[i].size();
        for (size_t k = 0; k < vvNearNeighbors[i].size(); k++) {
            const sMatch &s = vvNearNeighbors[i][k];
            idx[i * cap + k] = s.trainIdx, dist[i * cap + k] = s.distance, ncc[i * cap + k] = s.ncc;
        }
    }
    const int k = pagk_match_features(mN, (int32_t)cap, count.data(), idx.data(), dist.data(), ncc.data(), mbNCC ? 1 : 0, q.data(),
                                      t.data(), md.data(), mc.data());
    if (k < 0) fail("pagk_match_features", k);
    for (int r = 0; r < k; r++) vMatches.push_back(vvNearNeighbors[q[r]][0]);
}

// reference :859-939.  Steps 2 and 3 are one call: the searches, both MatchFeatures and the retry run on the device.
int GyroAidedTracker::SearchByGyroPredict()
{
    IntegrateGyroMeasurements();
    if (mType == GYRO_PREDICT)  // Step 1, :866-905
        GyroPredictFeatures();
    else {
        switch (mType) {
            case IMAGE_ONLY_OPTICAL_FLOW_CONSIDER_ILLUMINATION:
                mbHasGyroPredictInitial = false, mbConsiderIllumination = true, mbConsiderAffineDeformation = true,
                mbRegularizationPenalty = false;
                break;
            case GYRO_PREDICT_WITH_OPTICAL_FLOW_REFINED:
                mbHasGyroPredictInitial = true, mbConsiderIllumination = false, mbConsiderAffineDeformation = false,
                mbRegularizationPenalty = false;
                break;
            case GYRO_PREDICT_WITH_OPTICAL_FLOW_REFINED_CONSIDER_ILLUMINATION:
                mbHasGyroPredictInitial = true, mbConsiderIllumination = true, mbConsiderAffineDeformation = false,
                mbRegularizationPenalty = false;
                break;
            case GYRO_PREDICT_WITH_OPTICAL_FLOW_REFINED_CONSIDER_ILLUMINATION_DEFORMATION:
                mbHasGyroPredictInitial = true, mbConsiderIllumination = true, mbConsiderAffineDeformation = true,
                mbRegularizationPenalty = false;
                break;
            case GYRO_PREDICT_WITH_OPTICAL_FLOW_REFINED_CONSIDER_ILLUMINATION_DEFORMATION_REGULAR:
                mbHasGyroPredictInitial = true, mbConsiderIllumination = true, mbConsiderAffineDeformation = true,
                mbRegularizationPenalty = true;
                break;
            default:
                return -1;  // :899-902 "Unsupport type" (OPENCV_OPTICAL_FLOW_PYR_LK among them)
        }
        GyroPredictFeaturesAndOpticalFlowRefined();
    }
    const KeyArrays a = key_arrays(*this);
    const int m = (int)mvKeysCur.size();
    const pagk_image ref = image_of(mImgGrayRef), cur = image_of(mImgGrayCur);
    pagk_assoc_params ap;
    pagk_assoc_params_default(&ap);
    ap.th_ncc_high = TH_NCC_HIGH, ap.th_ncc_low = TH_NCC_LOW, ap.th_ratio = TH_RATIO, ap.use_ncc = mbNCC ? 1 : 0;
    std::vector<int32_t> q((size_t)mN + 1), t((size_t)mN + 1), count((size_t)mN + 1);
    std::vector<float> md((size_t)mN + 1), mc((size_t)mN + 1), flows(2 * (size_t)mN + 2);
    int32_t info[PAGK_ASSOC_INFO_WORDS] = {0};
    int cap = 64, k;
    std::vector<int32_t> idx;
    std::vector<float> dist, ncc;
    for (;;) {
        idx.assign((size_t)mN * cap + 1, -1), dist.assign((size_t)mN * cap + 1, 0.f), ncc.assign((size_t)mN * cap + 1, 0.f);
        k = pagk_search_gyro_predict(PatchMatch::Context(), &ap, &ref, &cur, mHalfPatchSize, mN, a.ref.data(), a.pred.data(),
                                     a.status.data(), a.affine.data(), m, a.cur.data(), a.cur_un.data(),
                                     mRadiusForFindNearNeighbor, cap, count.data(), idx.data(), dist.data(), ncc.data(), q.data(),
                                     t.data(), md.data(), mc.data(), flows.data(), info);
        if (k != PAGK_E_CAPACITY) break;
        for (int i = 0; i < mN; i++) cap = count[i] > cap ? count[i] : cap;  // count holds the sizes needed
    }
    if (k < 0) fail("pagk_search_gyro_predict", k);
    mvvNearNeighbors.assign(mN, std::vector<sMatch>());
    const float r1 = 1 * mRadiusForFindNearNeighbor;  // :811
    for (int i = 0; i < mN; i++)
        for (int c = 0; c < count[i]; c++) {
            const int j = idx[(size_t)i * cap + c];
            // a list found at level 2 was empty at level 1: its entries lie outside the level-1 square (:813-814)
            const cv::Point2f dpt = mvPtPredictUn[i] - mvKeysCurUn[j].pt;
            const int level = (std::fabs(dpt.x) > r1 || std::fabs(dpt.y) > r1) ? 2 : 1;
            mvvNearNeighbors[i].push_back(sMatch(i, j, dist[(size_t)i * cap + c], ncc[(size_t)i * cap + c], level));
        }
    mvMatches.clear();
    for (int r = 0; r < k; r++) mvMatches.push_back(mvvNearNeighbors[q[r]][0]);
    mvFlowsErrorUn.assign(mN, cv::Point2f(0, 0));  // Step 3, :928-933
    for (int i = 0; i < mN; i++) mvFlowsErrorUn[i] = cv::Point2f(flows[2 * i], flows[2 * i + 1]);
    return (int)mvMatches.size();
}

// reference :1017-1136.  cv::calcOpticalFlowPyrLK and cv::BFMatcher::radiusMatch are the library's definitions
// (include/pagk.h), not OpenCV's arithmetic.  The reference appends to mvMatches and mvDisparities; on a fresh tracker,
// which is how it is used, that is what is left here: both are cleared first.
int GyroAidedTracker::SearchByOpencvKLT()
{
    if (mImgGrayRef.empty() || mImgGrayCur.empty()) return -1;  // :1021-1025
    const size_t n = mvKeysRef.size(), m = mvKeysCur.size();
    std::vector<float> kr(2 * n + 2, 0.f), kc(2 * m + 2, 0.f), ptOut(2 * n + 2, 0.f), md(n + 1), err(n + 1, 0.f);
    std::vector<cv::uchar> status(n + 1, 0);
    std::vector<int32_t> q(n + 1), t(n + 1);
    std::vector<double> disp(n + 1);
    for (size_t i = 0; i < n; i++) kr[2 * i] = mvKeysRef[i].pt.x, kr[2 * i + 1] = mvKeysRef[i].pt.y;  // :1028-1030
    for (size_t j = 0; j < m; j++) kc[2 * j] = mvKeysCur[j].pt.x, kc[2 * j + 1] = mvKeysCur[j].pt.y;  // :1031-1033
    pagk_lk_params lk;
    pagk_lk_params_default(&lk);  // maxLevel 2, (COUNT + EPS, 30, 0.01), minEigThreshold 1e-4, 12.0 (:1036-1048)
    lk.half_patch = mHalfPatchSize;
    pagk_assoc_params ap;
    pagk_assoc_params_default(&ap);  // maxDistance 4, ratio 0.7, filterOutFactor 1.5 (:1066, :1081, :1115)
    const pagk_image ref = image_of(mImgGrayRef), cur = image_of(mImgGrayCur);
    const int k = pagk_search_klt(PatchMatch::Context(), &lk, &ap, &ref, &cur, (int32_t)n, kr.data(), (int32_t)m, kc.data(),
                                  ptOut.data(), status.data(), err.data(), q.data(), t.data(), md.data(), disp.data(), nullptr,
                                  nullptr, nullptr);
    if (k < 0) fail("pagk_search_klt", k);
    mvPtPredict.resize(n), mvStatus.resize(n), mvError.resize(n);
    for (size_t i = 0; i < n; i++) {  // :1041-1057
        mvPtPredict[i] = cv::Point2f(ptOut[2 * i], ptOut[2 * i + 1]);
        mvStatus[i] = status[i];
        mvError[i] = err[i];
    }
    mvMatches.clear(), mvDisparities.clear();
    for (int r = 0; r < k; r++) {
        mvMatches.push_back(sMatch(q[r], t[r], md[r]));  // :1092
        mvDisparities.push_back(disp[r]);                // :1100
    }
    return (int)mvMatches.size();
}

// ---- Step 2: geometry validation (reference :429-480) ----------------------------------------------
namespace {
GyroAidedTracker::ModelFitter &model_fitter()
{
    static GyroAidedTracker::ModelFitter f;
    return f;
}
}  // namespace

void GyroAidedTracker::SetModelFitter(ModelFitter fitter) { model_fitter() = std::move(fitter); }

int GyroAidedTracker::GeometryValidation()
{
    if (!model_fitter()) {  // the fits on the device (:429-480, 589-768)
        auto t0 = std::chrono::steady_clock::now();
        std::vector<float> p1(2 * (size_t)mN + 2), p2(2 * (size_t)mN + 2);
        std::vector<cv::uchar> status(mN ? mN : 1);
        for (int i = 0; i < mN; i++) {
            p1[2 * i] = mvKeysRefUn[i].pt.x, p1[2 * i + 1] = mvKeysRefUn[i].pt.y;
            p2[2 * i] = mvPtPredictUn[i].x, p2[2 * i + 1] = mvPtPredictUn[i].y;
            status[i] = mvStatus[i];
        }
        pagk_fit_params fp;
        pagk_fit_params_default(&fp);
        fp.seed = mFitSeed;
        float score = 0;
        int cnt_inlier = pagk_geometry_validation_fit(PatchMatch::Context(), &fp, mN, p1.data(), p2.data(),
                                                      status.data(), 1.0f, &score);
        if (cnt_inlier < 0)
            throw std::runtime_error(std::string("pagk_geometry_validation_fit failed: ") + pagk_strerror(cnt_inlier));
        for (int i = 0; i < mN; i++) mvStatus[i] = status[i];  // :472-476
        mTrackScore = score;
        mTimeCostGeometryValidation = std::chrono::duration<float>(std::chrono::steady_clock::now() - t0).count();
        mTImeCostTotalFeatureTrack =
            mTimeCostGyroPredict + mTimeCostOptFlow + mTimeCostOptFlowResultFilterOut + mTimeCostGeometryValidation;
        return cnt_inlier;
    }
    std::vector<cv::Point2f> vPts1, vPts2;  // :433-440
    for (size_t i = 0, iend = mvKeysRefUn.size(); i < iend; i++)
        if (mvStatus[i]) {
            vPts1.push_back(mvKeysRefUn[i].pt);
            vPts2.push_back(mvPtPredictUn[i]);
        }
    double H21[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, H12[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, F21[9] = {0};
    if (vPts1.size() > 8 && !model_fitter()(vPts1, vPts2, H21, H12, F21))  // :445, :596, :699
        throw std::runtime_error("GyroAidedTracker::GeometryValidation(): model fit failed");
    return GeometryValidation(H21, H12, F21);
}

int GyroAidedTracker::GeometryValidation(const double *H21, const double *H12, const double *F21, float sigma)
{
    auto t0 = std::chrono::steady_clock::now();
    std::vector<float> p1(2 * (size_t)mN + 2), p2(2 * (size_t)mN + 2);
    std::vector<cv::uchar> status(mN ? mN : 1);
    for (int i = 0; i < mN; i++) {
        p1[2 * i] = mvKeysRefUn[i].pt.x, p1[2 * i + 1] = mvKeysRefUn[i].pt.y;
        p2[2 * i] = mvPtPredictUn[i].x, p2[2 * i + 1] = mvPtPredictUn[i].y;
        status[i] = mvStatus[i];
    }
    float score = 0;
    int cnt_inlier = pagk_geometry_validation(PatchMatch::Context(), H21, H12, F21, mN, p1.data(), p2.data(),
                                              status.data(), sigma, &score);
    if (cnt_inlier < 0)
        throw std::runtime_error(std::string("pagk_geometry_validation failed: ") + pagk_strerror(cnt_inlier));
    for (int i = 0; i < mN; i++) mvStatus[i] = status[i];  // :472-476  outliers marked
    mTrackScore = score;
    mTimeCostGeometryValidation = std::chrono::duration<float>(std::chrono::steady_clock::now() - t0).count();
    mTImeCostTotalFeatureTrack =
        mTimeCostGyroPredict + mTimeCostOptFlow + mTimeCostOptFlowResultFilterOut + mTimeCostGeometryValidation;  // :483
    return cnt_inlier;
}
