// Stand-in for the reference's include/gyro_aided_tracker.h, found before it by include order
// (-I oracle/ref_shim -I $(REFERENCE)/include).
//
// TEST INFRASTRUCTURE (oracle/README.md, "The reference's own text, compiled").  PatchMatch reads its inputs from public
// data members of the tracker and writes its six result vectors back into it; this class is that state and nothing else.
// Which program uses which header: oracle/_ref/ref_patchmatch (ref_patchmatch.cpp, src/patch_match.cpp, src/utils.cpp) is
// compiled with -I oracle/ref_shim first and sees THIS class.  oracle/_ref/ref_tracker (ref_tracker.cpp and the same two
// sources with src/gyro_aided_tracker.cpp) puts the reference's include/ first and sees the reference's OWN
// include/gyro_aided_tracker.h: there the real class -- the gyro prediction, Step 3, the geometry scoring, the searches --
// is compiled and pinned (tests/test_reference_tracker_cpu.py).
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
