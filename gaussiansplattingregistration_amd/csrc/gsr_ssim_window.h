// gsr_ssim_window.h -- the SSIM window of the library, built once on the host: gsr_image_metrics (raster.hip) and gsr_loss_l1_dssim
// (imgloss.hip) hand the same eleven float64 taps to their kernels by value.
#pragma once
#include <math.h>

namespace gsr {

constexpr int SSIM_WIN = 11;                // taps; the 2-D window is the outer product of the normalised 1-D one
constexpr double SSIM_SIGMA = 1.5;
constexpr double SSIM_C1 = 0.01 * 0.01, SSIM_C2 = 0.03 * 0.03;

struct SsimWindow { double w[SSIM_WIN]; };

// w[j] = exp(-(j - 5)^2 / (2 sigma^2)), divided by their sum taken in ascending j
inline SsimWindow ssim_window() {
    SsimWindow win;
    double sum = 0.0;
    for (int j = 0; j < SSIM_WIN; ++j) {
        win.w[j] = exp(-(double)((j - SSIM_WIN / 2) * (j - SSIM_WIN / 2)) / (2.0 * SSIM_SIGMA * SSIM_SIGMA));
        sum += win.w[j];
    }
    for (int j = 0; j < SSIM_WIN; ++j) win.w[j] /= sum;
    return win;
}

}  // namespace gsr
