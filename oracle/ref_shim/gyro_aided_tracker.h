// Stand-in for the reference's include/gyro_aided_tracker.h, found before it by include order
// (-I oracle/ref_shim -I $(REFERENCE)/include).
//
// TEST INFRASTRUCTURE (oracle/README.md, "The reference's own text, compiled").  PatchMatch reads its inputs from public
// data members of the tracker and writes its six result vectors back into it; this class is that state and nothing else.
// The real class (src/gyro_aided_tracker.cpp: the gyro prediction, Step 3, the geometry scoring) needs imu_types, glog and
// a dozen more OpenCV routines, and is not compiled: everything it computes stays unpinned.
#ifndef PAGK_REF_SHIM_GYRO_AIDED_TRACKER_H
#define PAGK_REF_SHIM_GYRO_AIDED_TRACKER_H

#include <vector>

#include <opencv2/opencv.hpp>

class GyroAidedTracker {
public:
    // read by PatchMatch
    cv::Mat mImgGrayRef, mImgGrayCur;
    std::vector<cv::KeyPoint> mvKeysRef, mvKeysRefUn;
    std::vector<cv::Point2f> mvPtPredict, mvPtPredictUn;
    std::vector<uchar> mvStatus;
    std::vector<cv::Mat> mvAffineDeformationMatrix;
    cv::Mat mK, mDistCoef;
    // written by PatchMatch::SetMatcher
    std::vector<cv::Point2f> mvPtPredictAfterPatchMatched, mvPtPredictAfterPatchMatchedUn;
    std::vector<uchar> mvStatusAfterPatchMatched;
    std::vector<double> mvPixelErrorsOfPatchMatched;
    std::vector<double> mvDistanceBetweenPredictedAndPatchMatched;
    std::vector<float> mvNccAfterPatchMatched;
};

#endif
