// Frame ingest, the first stage (every frame passes through it before anything else): a raw 8-bit camera frame -> the planar
// float image of a KeyFrame, and a raw 16-bit depth frame -> metres -- data/tum_undistort.py:113,127-130 (cv2.undistort, margin
// crop, BGR -> RGB), data/image_transforms.py:36-60 (initUndistortRectifyMap + remap), tool/etc.py image_tt, frontend/
// process_frame.py:170-189 _downsample_to_target, data/tum_undistort.py:16-36 (DepthScale, DepthFilter), odometery/odometery.py:152-156.
//
// Image.  An output pixel is F.interpolate(bilinear, align_corners=False) of the cropped undistorted frame: two rows and two
// columns of it, <= 4 cropped pixels.  A cropped pixel is the bilinear sample (zero border) of the raw frame at its map
// position, <= 4 raw pixels: <= 16 three-byte taps per output pixel, each with the product of its four weights.  The map
// (OpenCV's initUndistortRectifyMap with R = I and newCameraMatrix = K, rational model) and every weight are evaluated in
// float64 per cropped pixel -- a float32 map is 1e-4 px off at 640 px -- and there is no map table: it would be 8 B a pixel
// against the 3 B of the image it indexes.  The map is formed as the pixel plus a displacement, (u, v) + f (x'' - x), so that
// without distortion a pixel maps onto itself EXACTLY: f ((u - c) / f) + c is u only to a rounding, and a weight of 1e-14 on
// a neighbour already turns a 0 into 1e-16.  The taps are summed in float64, rounded to float32 once and DIVIDED by 255.0f,
// so with every weight 0 or 1 the result is image_tt's, bit for bit.  Taps of weight exactly 0 are not loaded.  Neighbouring
// lanes read neighbouring raw bytes; a 0.9 MB frame sits in L2.
//
// Depth.  One gather per output pixel: d = (float)v * scale (float32, numpy's DepthScale), d > max_depth -> 0, crop, torch's
// nearest rule src = min((int)floorf(dst * ((float)in / out)), in - 1) (the identity when in == out).
#include <math.h>
#include "sp_device.h"

namespace {

constexpr int FI_COLS = 64;            // one wave per workgroup: 288 output columns fill 4.5 waves, not 1.1 workgroups of 256

struct FrameArgs {                     // by value in the kernel arguments
    SpCamera cam;
    int32_t H, W, top, left, Hc, Wc, Ho, Wo, bgr;
};

struct DepthArgs {
    int32_t H, W, top, left, Hc, Wc, Ho, Wo;
    float scale, max_depth;
};

// F.interpolate(bilinear, align_corners=False) along one axis: source indices i0 <= i1 and the weight of i1
__device__ __forceinline__ void resize_taps(int dst, int in, int out, int& i0, int& i1, double& w1) {
    const double s = fmax((dst + 0.5) * in / out - 0.5, 0.0);
    i0 = (int)s;                                                   // s >= 0: floor; s < in - 0.5
    i1 = min(i0 + 1, in - 1);
    w1 = s - i0;
}

// grid (ceil(Wo / FI_COLS), Ho, B), block FI_COLS: thread = one output pixel, all three channels
__global__ __launch_bounds__(FI_COLS) void k_frame_ingest(const uint8_t* __restrict__ raw, const FrameArgs g, float* __restrict__ out) {
    const int b = blockIdx.x * FI_COLS + threadIdx.x, a = blockIdx.y;
    if (b >= g.Wo) return;
    const SpCamera& k = g.cam;
    const uint8_t* frame = raw + (size_t)blockIdx.z * g.H * g.W * 3;
    int ci[2], cj[2];
    double wi1, wj1;
    resize_taps(a, g.Hc, g.Ho, ci[0], ci[1], wi1);
    resize_taps(b, g.Wc, g.Wo, cj[0], cj[1], wj1);
    const double wi[2] = {1.0 - wi1, wi1}, wj[2] = {1.0 - wj1, wj1};
    double x[2], y[2];                                             // normalised coordinates of the two cropped rows / columns
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        y[t] = ((ci[t] + g.top) - k.cy) / k.fy;
        x[t] = ((cj[t] + g.left) - k.cx) / k.fx;
    }
    double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) {
            const double wc = wi[ti] * wj[tj];
            if (wc == 0.0) continue;
            const double xx = x[tj], yy = y[ti], r2 = xx * xx + yy * yy;
            // the map as a displacement, m = (u, v) + f (x'' - x): kr - 1 = (numerator - denominator) / denominator
            const double up = ((k.k3 * r2 + k.k2) * r2 + k.k1) * r2, down = ((k.k6 * r2 + k.k5) * r2 + k.k4) * r2;
            const double dk = (up - down) / (1.0 + down);
            const double dx = xx * dk + 2.0 * k.p1 * xx * yy + k.p2 * (r2 + 2.0 * xx * xx);
            const double dy = yy * dk + k.p1 * (r2 + 2.0 * yy * yy) + 2.0 * k.p2 * xx * yy;
            const double mx = (cj[tj] + g.left) + k.fx * dx, my = (ci[ti] + g.top) + k.fy * dy;
            if (!(mx > -1.0 && mx < g.W && my > -1.0 && my < g.H)) continue;       // no tap inside the frame (or a NaN map)
            const double fx0 = floor(mx), fy0 = floor(my);
            const int x0 = (int)fx0, y0 = (int)fy0;                               // in -1 .. W - 1, -1 .. H - 1
            const double ax = mx - fx0, ay = my - fy0;
            const double wx[2] = {1.0 - ax, ax}, wy[2] = {(1.0 - ay) * wc, ay * wc};
#pragma unroll
            for (int sy = 0; sy < 2; ++sy) {
#pragma unroll
                for (int sx = 0; sx < 2; ++sx) {
                    const double w = wy[sy] * wx[sx];
                    const int px = x0 + sx, py = y0 + sy;
                    if (w == 0.0 || px < 0 || px >= g.W || py < 0 || py >= g.H) continue;
                    const uint8_t* p = frame + ((size_t)py * g.W + px) * 3;
                    acc[0] = fma(w, (double)p[0], acc[0]);
                    acc[1] = fma(w, (double)p[1], acc[1]);
                    acc[2] = fma(w, (double)p[2], acc[2]);
                }
            }
        }
    }
    const size_t plane = (size_t)g.Ho * g.Wo, at = (size_t)blockIdx.z * 3 * plane + (size_t)a * g.Wo + b;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[at + (g.bgr ? 2 - c : c) * plane] = __fdiv_rn((float)acc[c], 255.0f);
}

// the same grid: thread = one output pixel
__global__ __launch_bounds__(FI_COLS) void k_depth_ingest(const uint16_t* __restrict__ raw, const DepthArgs g, float* __restrict__ out) {
    const int b = blockIdx.x * FI_COLS + threadIdx.x, a = blockIdx.y;
    if (b >= g.Wo) return;
    const int i = min((int)floorf(a * ((float)g.Hc / (float)g.Ho)), g.Hc - 1);
    const int j = min((int)floorf(b * ((float)g.Wc / (float)g.Wo)), g.Wc - 1);
    const uint16_t v = raw[((size_t)blockIdx.z * g.H + (i + g.top)) * g.W + (j + g.left)];
    const float d = __fmul_rn((float)v, g.scale);
    out[((size_t)blockIdx.z * g.Ho + a) * g.Wo + b] = d > g.max_depth ? 0.f : d;
}

int frame_sizes(int B, int H, int W, int top, int left, int Hc, int Wc, int Ho, int Wo) {
    if (B <= 0 || H <= 0 || W <= 0 || Hc <= 0 || Wc <= 0 || Ho <= 0 || Wo <= 0) return SP_EINVAL;
    if (top < 0 || left < 0 || (long long)top + Hc > H || (long long)left + Wc > W) return SP_EINVAL;
    if (W > 32767 || (long long)H * W >= (1LL << 31) || B > 65535 || Ho > 65535) return SP_ELIMIT;
    return 0;
}

}  // namespace

extern "C" {

int sp_frame_ingest(const uint8_t* raw, int B, int H, int W, const SpCamera* cam, int top, int left, int Hc, int Wc, int Ho, int Wo,
                    int bgr, float* out, void* stream) {
    if (!raw || !cam || !out || (const void*)out == (const void*)raw) return SP_EINVAL;
    const int rc = frame_sizes(B, H, W, top, left, Hc, Wc, Ho, Wo);
    if (rc) return rc;
    if (!(isfinite(cam->fx) && isfinite(cam->fy) && cam->fx > 0.0 && cam->fy > 0.0)) return SP_ELIMIT;
    FrameArgs g;
    g.cam = *cam;
    g.H = H; g.W = W; g.top = top; g.left = left; g.Hc = Hc; g.Wc = Wc; g.Ho = Ho; g.Wo = Wo; g.bgr = bgr != 0;
    hipLaunchKernelGGL(k_frame_ingest, dim3((Wo + FI_COLS - 1) / FI_COLS, Ho, B), dim3(FI_COLS), 0, static_cast<hipStream_t>(stream), raw, g,
                       out);
    SP_CHECK_LAUNCH();
    return 0;
}

int sp_depth_ingest(const uint16_t* raw, int B, int H, int W, float scale, float max_depth, int top, int left, int Hc, int Wc, int Ho,
                    int Wo, float* out, void* stream) {
    if (!raw || !out || (const void*)out == (const void*)raw) return SP_EINVAL;
    const int rc = frame_sizes(B, H, W, top, left, Hc, Wc, Ho, Wo);
    if (rc) return rc;
    DepthArgs g;
    g.H = H; g.W = W; g.top = top; g.left = left; g.Hc = Hc; g.Wc = Wc; g.Ho = Ho; g.Wo = Wo; g.scale = scale; g.max_depth = max_depth;
    hipLaunchKernelGGL(k_depth_ingest, dim3((Wo + FI_COLS - 1) / FI_COLS, Ho, B), dim3(FI_COLS), 0, static_cast<hipStream_t>(stream), raw, g,
                       out);
    SP_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
