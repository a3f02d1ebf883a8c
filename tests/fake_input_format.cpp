// Test infrastructure (tests/test_queue_input_format_host.py): the input-format setting of a context of the recording stand-in runtime
// (tests/fake_runtime.cpp), which predates it.  The queue keeps the setting in CtxHooks::input_format (ugsm_internal.hpp); these two calls
// set and read it there, as ugsm_set_input_format / ugsm_get_input_format do in the real runtime.
#include "../ug_stereomatcher_amd/csrc/ugsm_internal.hpp"

extern "C" {
__attribute__((visibility("default"))) int ugsm_fake_set_input_format(ugsm_ctx *ctx, int format)
{
    if (ugsm::input_bpp(format) < 0) return UGSM_ERR_BAD_ARG;
    ugsm::ctx_hooks(ctx).input_format = format;
    return UGSM_OK;
}
__attribute__((visibility("default"))) int ugsm_fake_get_input_format(ugsm_ctx *ctx) { return ugsm::ctx_hooks(ctx).input_format; }
}
