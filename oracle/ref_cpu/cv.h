/*
 * cv.h -- stand-in for the handful of old OpenCV C names that the reference's host driver mentions, for its CPU build (see
 * cuda_runtime.h beside this file).  TEST INFRASTRUCTURE ONLY; not the declaration-only files of tests/ros_stubs/.
 *
 * The driver's debug image writers are commented out; what is left alive is a declared IplImage pointer per function and one
 * cvReleaseImage(&p) of a pointer that was never set (hierarchicalDisparity).  No image is ever created through this header's
 * cvCreateImage in a run, so cvReleaseImage has nothing of its own to release and touches nothing: freeing through an unset pointer
 * is the one thing it must not do.  Nothing is read from or written to disk.
 */
#ifndef UGSM_REF_CPU_CV_H
#define UGSM_REF_CPU_CV_H

#include <cstdlib>

typedef unsigned char uchar;

struct CvSize {
    int width, height;
};
inline CvSize cvSize(int width, int height) { return {width, height}; }

struct IplImage {
    int nChannels, depth, width, height, widthStep;
    char *imageData;
};

enum { CV_LOAD_IMAGE_ANYCOLOR = 4 };

inline IplImage *cvCreateImage(CvSize size, int depth, int channels)
{
    const int step = (size.width * channels * (depth / 8) + 3) & ~3; /* rows are padded to four bytes */
    return new IplImage{channels, depth, size.width, size.height, step, (char *)std::calloc((size_t)step * size.height, 1)};
}
inline void cvReleaseImage(IplImage **) {}
inline int cvSaveImage(const char *, const IplImage *) { return 0; }
inline IplImage *cvLoadImage(const char *, int) { return nullptr; }

#endif
