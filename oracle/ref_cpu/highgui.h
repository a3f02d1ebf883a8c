/* highgui.h -- stand-in: the image reading and writing names live in cv.h beside this file.  TEST INFRASTRUCTURE ONLY. */
#ifndef UGSM_REF_CPU_HIGHGUI_H
#define UGSM_REF_CPU_HIGHGUI_H
#include "cv.h"
#endif
