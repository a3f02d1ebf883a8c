// ugsm_no_dev.cpp -- linked into libugsm.so only, where libugsm_dev.so links csrc/dev/: the product's answer to "which library is this", and
// no-op stand-ins for the development launchers, which no configuration that ugsm_create accepts here reaches (ugsm_launch.hpp).
#include "ugsm_launch.hpp"

namespace ugsm {

const bool kDevLib = false;
void launch_blur_decimate_ref(hipStream_t, const float *, int, int, float *, int, int, float) {}
void launch_sqblur_clamp_ref(hipStream_t, Img3, int, int, float *) {}
void launch_warp_ref(hipStream_t, Img3, const float *, int, int, float *) {}
void launch_cost_ref(hipStream_t, Img3, const float *, const float *, const float *, const float *, float *, int, int, float, int, float *) {}
void launch_smooth_pass_ref(hipStream_t, const float *, float *, int, int) {}
void launch_box_ref(hipStream_t, const float *, float *, int, int) {}
void launch_cost_fused(hipStream_t, Img3, Img3, const float *, const float *, float *, int, int, float, int) {}

}  // namespace ugsm
