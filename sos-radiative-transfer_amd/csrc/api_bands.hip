// Band integration (include/sosrt.h): Planck band radiances on the device and the weighted sum over the
// spectral points of a batch; and the brightness temperature of a band-summed radiance, the inverse of the
// Planck stage.  Three stages beside the solve: of the handle they use L (the Planck stage) and the stream, and like
// every stage they end the profiling slots' run of adjacent launches; nothing of the solve state is read or written -- columns,
// resident field, order targets and phase state stay as they were.  Host code.
#include <hip/hip_runtime.h>

#include <cmath>

#include "bands.hpp"
#include "brightness.hpp"
#include "handle.hpp"

using namespace sosrt;

extern "C" {

int sosrt_planck_bands_dev(sosrt_t* h, int C, int K, const double* d_T, const double* d_T_surface, const double* nu_lo,
                           const double* nu_hi, int normalise, double* d_planck_out, double* d_planck_surface_out,
                           double* d_scale_out) {
    // every check comes before the first launch, so a refused call writes nothing
    if (int e = need_gpu(h)) return e;
    if (C < 1 || K < 1) return fail(SOSRT_E_INVALID, "sosrt_planck_bands_dev: C=%d columns, K=%d bands: both must be >= 1", C, K);
    if (normalise != 0 && normalise != 1) return fail(SOSRT_E_INVALID, "sosrt_planck_bands_dev: normalise=%d: must be 0 or 1", normalise);
    if (!d_T || !d_T_surface || !nu_lo || !nu_hi || !d_planck_out || !d_planck_surface_out)
        return fail(SOSRT_E_INVALID, "sosrt_planck_bands_dev: null argument");
    if (normalise && !d_scale_out)
        return fail(SOSRT_E_INVALID, "sosrt_planck_bands_dev: null d_scale_out: normalise=1 divides by the scale, which the caller needs back");
    for (int k = 0; k < K; ++k) {
        if (!(std::isfinite(nu_lo[k]) && std::isfinite(nu_hi[k]) && nu_lo[k] >= 0))
            return fail(SOSRT_E_INVALID, "sosrt_planck_bands_dev: band %d = [%g, %g] cm^-1: an edge must be finite and >= 0", k, nu_lo[k], nu_hi[k]);
        if (!(nu_hi[k] > nu_lo[k]))
            return fail(SOSRT_E_INVALID, "sosrt_planck_bands_dev: band %d = [%g, %g] cm^-1: nu_hi must be > nu_lo", k, nu_lo[k], nu_hi[k]);
    }
    HIPCHK(hipSetDevice(h->device));
    prof_break(h);
    const size_t CL = (size_t)C * h->L;
    for (int k0 = 0; k0 < K; k0 += kBandsPerLaunch) {
        const int nk = K - k0 < kBandsPerLaunch ? K - k0 : kBandsPerLaunch;
        BandEdges e;
        for (int j = 0; j < kBandsPerLaunch; ++j) { e.lo[j] = j < nk ? nu_lo[k0 + j] : 0; e.hi[j] = j < nk ? nu_hi[k0 + j] : 1; }
        launch_planck_bands(h->stream, C, nk, h->L, d_T, d_T_surface, e, normalise, d_planck_out + k0 * CL,
                            d_planck_surface_out + (size_t)k0 * C, d_scale_out ? d_scale_out + (size_t)k0 * C : nullptr);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

int sosrt_band_reduce_dev(sosrt_t* h, int C, int K, int M, const double* d_weight, const double* d_scale, const double* d_x,
                          double* d_out, int accumulate) {
    if (int e = need_gpu(h)) return e;
    if (C < 1 || K < 1 || M < 1)
        return fail(SOSRT_E_INVALID, "sosrt_band_reduce_dev: C=%d columns, K=%d points, M=%d values: all must be >= 1", C, K, M);
    if ((size_t)C * M > (size_t)0x7fffffff * kReduceBlock)
        return fail(SOSRT_E_INVALID, "sosrt_band_reduce_dev: C=%d x M=%d values are more than one launch takes", C, M);
    if (!d_x || !d_out) return fail(SOSRT_E_INVALID, "sosrt_band_reduce_dev: null argument");
    HIPCHK(hipSetDevice(h->device));
    prof_break(h);
    launch_band_reduce(h->stream, C, K, M, d_weight, d_scale, d_x, d_out, accumulate != 0);
    HIPCHK(hipGetLastError());
    return 0;
}

int sosrt_brightness_temperature_dev(sosrt_t* h, int C, int K, int M, const double* nu_lo, const double* nu_hi,
                                     const double* d_weight, const double* d_radiance, double* d_T_out) {
    // every check comes before the launch, so a refused call writes nothing
    if (int e = need_gpu(h)) return e;
    if (C < 1 || K < 1 || M < 1)
        return fail(SOSRT_E_INVALID, "sosrt_brightness_temperature_dev: C=%d columns, K=%d bands, M=%d values: all must be >= 1", C, K, M);
    if (K > kBandsPerLaunch)
        return fail(SOSRT_E_INVALID, "sosrt_brightness_temperature_dev: K=%d bands: at most %d (the sum over the bands sits inside "
                    "the iteration, so they cannot be split over launches)", K, kBandsPerLaunch);
    if ((size_t)C * M > (size_t)0x7fffffff * kBrightnessBlock)
        return fail(SOSRT_E_INVALID, "sosrt_brightness_temperature_dev: C=%d x M=%d values are more than one launch takes", C, M);
    if (!nu_lo || !nu_hi || !d_radiance || !d_T_out) return fail(SOSRT_E_INVALID, "sosrt_brightness_temperature_dev: null argument");
    for (int k = 0; k < K; ++k) {
        if (!(std::isfinite(nu_lo[k]) && std::isfinite(nu_hi[k]) && nu_lo[k] >= 0))
            return fail(SOSRT_E_INVALID, "sosrt_brightness_temperature_dev: band %d = [%g, %g] cm^-1: an edge must be finite and >= 0", k, nu_lo[k], nu_hi[k]);
        if (!(nu_hi[k] > nu_lo[k]))
            return fail(SOSRT_E_INVALID, "sosrt_brightness_temperature_dev: band %d = [%g, %g] cm^-1: nu_hi must be > nu_lo", k, nu_lo[k], nu_hi[k]);
    }
    HIPCHK(hipSetDevice(h->device));
    prof_break(h);
    BandEdges e;
    for (int j = 0; j < kBandsPerLaunch; ++j) { e.lo[j] = j < K ? nu_lo[j] : 0; e.hi[j] = j < K ? nu_hi[j] : 1; }
    launch_brightness_temperature(h->stream, C, K, M, e, d_weight, d_radiance, d_T_out);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"
