/*
 * cv_bridge/cv_bridge.h -- stand-in for the image type that the reference's host driver takes, for its CPU build (see
 * ../cuda_runtime.h).  TEST INFRASTRUCTURE ONLY; not the declaration-only file of tests/ros_stubs/.  The driver reads four fields
 * of a shared pointer's image: the first byte, the number of rows and columns, and the distance in bytes between two rows.
 */
#ifndef UGSM_REF_CPU_CV_BRIDGE_H
#define UGSM_REF_CPU_CV_BRIDGE_H

#include <cstddef>
#include <memory>

namespace cv {
struct Mat {
    unsigned char *data = nullptr;
    int rows = 0, cols = 0;
    size_t step = 0;
};
}

namespace cv_bridge {
struct CvImage {
    cv::Mat image;
};
typedef std::shared_ptr<CvImage> CvImagePtr;
}

#endif
