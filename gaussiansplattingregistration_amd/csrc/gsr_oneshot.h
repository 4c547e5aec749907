// gsr_oneshot.h -- the device memory of a stateless one-shot entry point (gsr_plane_score, gsr_fpfh, gsr_voxel_down_sample, ...):
// caller arrays that are all on the host or all on the device, scratch, results copied back for host callers, one wait, everything
// freed.  The contexts (gsr_hem_*, gsr_icp_*, gsr_raster_*) keep grow-only DevBuf workspaces as members, which live as long as the
// context does, and do not use this.
#pragma once
#include <vector>

#include "gsr_common.h"
#include "gsr_model_arrays.h"

namespace gsr {

// the device a one-shot call runs on: checked and made current
inline int32_t open_device(int32_t device, const char* who) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(GSR_E_NO_DEVICE, "%s: no HIP device visible (this backend has no CPU fallback)", who);
    if (device < 0 || device >= ndev) return fail(GSR_E_INVALID, "%s: device %d out of range", who, device);
    GSR_HIP(hipSetDevice(device));
    return GSR_OK;
}

// Owner of everything one call allocates on the device.  The destructor WAITS FOR THE STREAM AND THEN FREES, on every exit, the
// early returns of GSR_HIP / GSR_TRY included: that wait is what makes an asynchronous copy into the caller's frame (a local, a
// std::vector declared before the OneShot) or out of a staged buffer safe when the function leaves before its own wait.  There is
// no release without the wait: the wait is the destructor's body and the buffers are members, which C++ destroys after the body.
struct OneShot {
    OneShot(hipStream_t stream, bool on_device, const char* who) : st(stream), on_device(on_device), who(who) {}
    OneShot(const OneShot&) = delete;
    OneShot& operator=(const OneShot&) = delete;
    ~OneShot() {
        (void)hipStreamSynchronize(st);
    }

    // plain device scratch of `bytes` bytes
    template <typename T> int32_t scratch(size_t bytes, T** dev) {
        owned.emplace_back();
        GSR_TRY(owned.back().reserve(bytes));
        *dev = owned.back().as<T>();
        return GSR_OK;
    }
    // device view of a caller input: the array itself (on_device, or NULL) or a staged copy, enqueued on the stream
    template <typename T> int32_t in(const T* p, size_t bytes, const T** dev) {
        if (!p || on_device) { *dev = p; return GSR_OK; }
        T* d = nullptr;
        GSR_TRY(scratch(bytes, &d));
        GSR_HIP(hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, st));
        *dev = d;
        return GSR_OK;
    }
    // device destination of a caller output: the array itself (on_device, or NULL) or a buffer that finish() copies back
    template <typename T> int32_t out(T* p, size_t bytes, T** dev) {
        if (!p || on_device) { *dev = p; return GSR_OK; }
        GSR_TRY(scratch(bytes, dev));
        backs.push_back({p, *dev, bytes});
        return GSR_OK;
    }
    // waits for the stream; a launch error so far, `e` or the wait's own becomes "<who>: <HIP's text>" (a mid-call read-back ends here)
    int32_t wait(hipError_t e = hipGetLastError()) {
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        return e == hipSuccess ? GSR_OK : fail(GSR_E_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    // the end of a successful call: launch errors, the recorded copy-backs, the wait
    int32_t finish() {
        hipError_t e = hipGetLastError();
        for (const Back& b : backs)
            if (e == hipSuccess) e = hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, st);
        backs.clear();
        return wait(e);
    }

    const hipStream_t st;
    const bool on_device;
    const char* const who;

private:
    struct Back { void* host; const void* dev; size_t bytes; };
    std::vector<DevBuf> owned;
    std::vector<Back> backs;
};

// ---- whole models (gsr_model_view) in a one-shot call; width[] / used[] are model_layout's
// device views of the used arrays of an input model (NULL for an unused array and for a model without rows)
inline int32_t model_in(OneShot& os, const gsr_model_view* v, const size_t width[GSR_MODEL_NARR], const bool used[GSR_MODEL_NARR], const float* dev[GSR_MODEL_NARR]) {
    for (int k = 0; k < GSR_MODEL_NARR; ++k) {
        dev[k] = nullptr;
        if (used[k] && v->n > 0) GSR_TRY(os.in((const float*)model_array(v, k), (size_t)v->n * width[k] * 4, &dev[k]));
    }
    return GSR_OK;
}
// device destinations of the used arrays of an output model of `rows` rows: the caller's on the device, else scratch of that capacity.
// The row count is known only after the kernels, so a host caller's rows come back through model_copy_back, not through finish().
inline int32_t model_out(OneShot& os, const gsr_model_view* out, int64_t rows, const size_t width[GSR_MODEL_NARR], const bool used[GSR_MODEL_NARR], float* dev[GSR_MODEL_NARR]) {
    for (int k = 0; k < GSR_MODEL_NARR; ++k) {
        dev[k] = nullptr;
        if (!used[k] || rows == 0) continue;
        if (os.on_device) dev[k] = model_array(out, k);
        else GSR_TRY(os.scratch((size_t)rows * width[k] * 4, &dev[k]));
    }
    return GSR_OK;
}
// the first n_rows rows of every staged array to a host caller: n_rows rows, not the capacity
inline int32_t model_copy_back(OneShot& os, const gsr_model_view* out, float* const dev[GSR_MODEL_NARR], int64_t n_rows, const size_t width[GSR_MODEL_NARR]) {
    for (int k = 0; k < GSR_MODEL_NARR && !os.on_device; ++k)
        if (dev[k] && n_rows > 0) GSR_HIP(hipMemcpyAsync(model_array(out, k), dev[k], (size_t)n_rows * width[k] * 4, hipMemcpyDeviceToHost, os.st));
    return GSR_OK;
}

}  // namespace gsr
