// dis_stabilize.cpp -- dis_motion_stabilize (include/dis_abi.h): the pair
// models of a video composed into a camera path, the path smoothed by a
// truncated Gaussian, and per frame the model that warps the frame onto the
// smoothed path. Host only (no GPU), like dis_denoise_weights: n_frames * 6
// numbers in, as many out. No reference counterpart: the reference computes a
// flow and never applies it.
//
// All of it is f64 with every operation rounded on its own, in the order the
// header states (this file is compiled with -ffp-contract=off), so
// tests/stabref.py restates it bit for bit in Python floats. A 2 x 3 matrix is
// six doubles m[0..5] = m00 m01 m02 m10 m11 m12, its third row 0 0 1 implied.
// dis_homography_stabilize is the same for eight-parameter models, with full
// 3 x 3 matrices (tests/homographyref.py restates it).
#include <cmath>
#include <cstdint>
#include <new>
#include <string>
#include <vector>

#include "dis_abi.h"
#include "dis_args.h"

namespace dis {
dis_status set_error(dis_status s, const std::string& msg);  // dis_runtime.hip
}

namespace {

struct Mat {
    double m[6];
};

constexpr Mat kIdentity = {{1.0, 0.0, 0.0, 0.0, 1.0, 0.0}};

// a . b: an entry is (a_i0*b_0j + a_i1*b_1j), + a_i2 for j = 2, left to right
Mat mul(const Mat& a, const Mat& b)
{
    Mat r;
    for (int i = 0; i < 2; ++i) {
        const double a0 = a.m[3 * i], a1 = a.m[3 * i + 1], a2 = a.m[3 * i + 2];
        r.m[3 * i] = a0 * b.m[0] + a1 * b.m[3];
        r.m[3 * i + 1] = a0 * b.m[1] + a1 * b.m[4];
        r.m[3 * i + 2] = (a0 * b.m[2] + a1 * b.m[5]) + a2;
    }
    return r;
}

// The matrix of one pair model; false when a parameter is not finite.
bool pair_matrix(const float* p, Mat* a)
{
    for (int i = 0; i < 6; ++i)
        if (!std::isfinite(p[i])) return false;
    *a = {{1.0 + (double)p[1], (double)p[2], (double)p[0], (double)p[4], 1.0 + (double)p[5], (double)p[3]}};
    return true;
}

// S^-1; false when the determinant is not finite or |det| <= 2^-20.
bool invert(const Mat& s, Mat* inv)
{
    const double det = s.m[0] * s.m[4] - s.m[1] * s.m[3];
    if (!std::isfinite(det) || std::fabs(det) <= 0x1p-20) return false;
    const double i00 = s.m[4] / det, i01 = -s.m[1] / det, i10 = -s.m[3] / det, i11 = s.m[0] / det;
    const double i02 = -(i00 * s.m[2] + i01 * s.m[5]);
    const double i12 = -(i10 * s.m[2] + i11 * s.m[5]);
    *inv = {{i00, i01, i02, i10, i11, i12}};
    return true;
}

// The eight-parameter family (dis_homography_stabilize): full 3 x 3 matrices,
// nine doubles row-major, kept at bottom-right 1.
struct Mat3 {
    double m[9];
};

constexpr Mat3 kIdentity3 = {{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}};

// a . b: an entry is (a_i0*b_0j + a_i1*b_1j) + a_i2*b_2j
Mat3 mul3(const Mat3& a, const Mat3& b)
{
    Mat3 r;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            r.m[3 * i + j] = (a.m[3 * i] * b.m[j] + a.m[3 * i + 1] * b.m[3 + j]) + a.m[3 * i + 2] * b.m[6 + j];
    return r;
}

// every entry divided by the bottom-right one
Mat3 normalise3(const Mat3& a)
{
    Mat3 r;
    const double w = a.m[8];
    for (int e = 0; e < 9; ++e) r.m[e] = a.m[e] / w;
    return r;
}

bool pair_matrix3(const float* p, Mat3* a)
{
    for (int i = 0; i < 8; ++i)
        if (!std::isfinite(p[i])) return false;
    *a = {{1.0 + (double)p[1], (double)p[2], (double)p[0], (double)p[4], 1.0 + (double)p[5], (double)p[3],
           (double)p[6], (double)p[7], 1.0}};
    return true;
}

// S^-1 = adj(S) / det; false when the determinant is not finite or |det| <= 2^-20.
bool invert3(const Mat3& s, Mat3* inv)
{
    const double* const m = s.m;
    const double k00 = m[4] * m[8] - m[5] * m[7], k01 = m[3] * m[8] - m[5] * m[6], k02 = m[3] * m[7] - m[4] * m[6];
    const double det = (m[0] * k00 - m[1] * k01) + m[2] * k02;
    if (!std::isfinite(det) || std::fabs(det) <= 0x1p-20) return false;
    *inv = {{k00 / det, (m[2] * m[7] - m[1] * m[8]) / det, (m[1] * m[5] - m[2] * m[4]) / det,
             (m[5] * m[6] - m[3] * m[8]) / det, (m[0] * m[8] - m[2] * m[6]) / det, (m[2] * m[3] - m[0] * m[5]) / det,
             k02 / det, (m[1] * m[6] - m[0] * m[7]) / det, (m[0] * m[4] - m[1] * m[3]) / det}};
    return true;
}

}  // namespace

extern "C" dis_status dis_homography_stabilize(const float* pair_params, int n_frames, int width, int height, int radius,
                                               float sigma, float zoom, float* corrections, uint8_t* status,
                                               int* replaced)
{
    if (!corrections) return dis::set_error(DIS_ERR_INVALID_ARGUMENT, "null pointer");
    if (const char* why = dis::check_stabilize(n_frames, width, height, radius, sigma, zoom))
        return dis::set_error(DIS_ERR_INVALID_ARGUMENT, why);
    if (n_frames > 1 && !pair_params) return dis::set_error(DIS_ERR_INVALID_ARGUMENT, "null pointer");
    dis::PairMessage msg;
    if (const char* why = dis::check_homography_stabilize_buffers(
            n_frames > 1 ? reinterpret_cast<uintptr_t>(pair_params) : 0, reinterpret_cast<uintptr_t>(corrections),
            reinterpret_cast<uintptr_t>(status), reinterpret_cast<uintptr_t>(replaced), n_frames, &msg))
        return dis::set_error(DIS_ERR_INVALID_ARGUMENT, why);
    const int n = n_frames;
    std::vector<Mat3> path;  // 72 bytes a frame
    std::vector<double> g;
    const int reach = radius < n - 1 ? radius : n - 1;  // no frame is further than n - 1 away
    try {
        path.resize((size_t)n);
        g.resize((size_t)reach + 1);
    } catch (const std::bad_alloc&) {
        return dis::set_error(DIS_ERR_OUT_OF_MEMORY, "no host memory for the path of n_frames frames");
    }
    int bad = 0;
    path[0] = kIdentity3;
    for (int k = 0; k + 1 < n; ++k) {
        Mat3 a;
        if (!pair_matrix3(pair_params + 8 * (size_t)k, &a)) {
            a = kIdentity3;
            ++bad;
        }
        path[k + 1] = normalise3(mul3(a, path[k]));
    }
    const double s2 = 2.0 * (double)sigma * (double)sigma;
    for (int d = 0; d <= reach; ++d) g[d] = (double)(float)std::exp(-((double)d * d) / s2);
    const double z = 1.0 / (double)zoom;
    const double cx = (width - 1) / 2.0, cy = (height - 1) / 2.0;
    const Mat3 Z = {{z, 0.0, cx * (1.0 - z), 0.0, z, cy * (1.0 - z), 0.0, 0.0, 1.0}};
    for (int k = 0; k < n; ++k) {
        const int lo = k - reach > 0 ? k - reach : 0, hi = k + reach < n - 1 ? k + reach : n - 1;
        Mat3 s = {{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};
        double wsum = 0.0;
        for (int j = lo; j <= hi; ++j) {
            const double w = g[j > k ? j - k : k - j];
            for (int e = 0; e < 9; ++e) s.m[e] = s.m[e] + w * path[j].m[e];
            wsum = wsum + w;
        }
        for (int e = 0; e < 9; ++e) s.m[e] = s.m[e] / wsum;
        float q[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        Mat3 inv;
        bool ok = invert3(s, &inv);
        if (ok) {
            const Mat3 m = normalise3(mul3(mul3(path[k], inv), Z));
            float r[8] = {(float)m.m[2], (float)(m.m[0] - 1.0), (float)m.m[1], (float)m.m[5],
                          (float)m.m[3], (float)(m.m[4] - 1.0), (float)m.m[6], (float)m.m[7]};
            for (int e = 0; e < 8; ++e) ok = ok && std::isfinite(r[e]);
            for (int e = 6; e < 8; ++e)
                if (r[e] == 0.0f) r[e] = 0.0f;  // a zero of either sign is written as +0.0f
            if (ok)
                for (int e = 0; e < 8; ++e) q[e] = r[e];
        }
        for (int e = 0; e < 8; ++e) corrections[8 * (size_t)k + e] = q[e];
        if (status) status[k] = ok ? 1 : 0;
    }
    if (replaced) *replaced = bad;
    return DIS_OK;
}

extern "C" dis_status dis_motion_stabilize(const float* pair_params, int n_frames, int width, int height, int radius,
                                           float sigma, float zoom, float* corrections, uint8_t* status, int* replaced)
{
    if (!corrections) return dis::set_error(DIS_ERR_INVALID_ARGUMENT, "null pointer");
    if (const char* why = dis::check_stabilize(n_frames, width, height, radius, sigma, zoom))
        return dis::set_error(DIS_ERR_INVALID_ARGUMENT, why);
    if (n_frames > 1 && !pair_params) return dis::set_error(DIS_ERR_INVALID_ARGUMENT, "null pointer");
    dis::PairMessage msg;
    if (const char* why = dis::check_stabilize_buffers(n_frames > 1 ? reinterpret_cast<uintptr_t>(pair_params) : 0,
                                                       reinterpret_cast<uintptr_t>(corrections),
                                                       reinterpret_cast<uintptr_t>(status),
                                                       reinterpret_cast<uintptr_t>(replaced), n_frames, &msg))
        return dis::set_error(DIS_ERR_INVALID_ARGUMENT, why);
    const int n = n_frames;
    // the path: C_0 = I, C_{k+1} = A_k . C_k (48 bytes a frame; the weights below: 8 bytes a frame at most)
    std::vector<Mat> path;
    std::vector<double> g;
    const int reach = radius < n - 1 ? radius : n - 1;  // no frame is further than n - 1 away
    try {
        path.resize((size_t)n);
        g.resize((size_t)reach + 1);
    } catch (const std::bad_alloc&) {
        return dis::set_error(DIS_ERR_OUT_OF_MEMORY, "no host memory for the path of n_frames frames");
    }
    int bad = 0;
    path[0] = kIdentity;
    for (int k = 0; k + 1 < n; ++k) {
        Mat a;
        if (!pair_matrix(pair_params + 6 * (size_t)k, &a)) {
            a = kIdentity;
            ++bad;
        }
        path[k + 1] = mul(a, path[k]);
    }
    // the weights, rounded as dis_denoise_weights rounds them
    const double s2 = 2.0 * (double)sigma * (double)sigma;
    for (int d = 0; d <= reach; ++d) g[d] = (double)(float)std::exp(-((double)d * d) / s2);
    const double z = 1.0 / (double)zoom;
    const double cx = (width - 1) / 2.0, cy = (height - 1) / 2.0;
    const Mat Z = {{z, 0.0, cx * (1.0 - z), 0.0, z, cy * (1.0 - z)}};
    for (int k = 0; k < n; ++k) {
        const int lo = k - reach > 0 ? k - reach : 0, hi = k + reach < n - 1 ? k + reach : n - 1;
        Mat s = {{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};
        double wsum = 0.0;
        for (int j = lo; j <= hi; ++j) {
            const double w = g[j > k ? j - k : k - j];
            for (int e = 0; e < 6; ++e) s.m[e] = s.m[e] + w * path[j].m[e];
            wsum = wsum + w;
        }
        for (int e = 0; e < 6; ++e) s.m[e] = s.m[e] / wsum;
        float q[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        Mat inv;
        bool ok = invert(s, &inv);
        if (ok) {
            const Mat m = mul(mul(path[k], inv), Z);
            const float r[6] = {(float)m.m[2], (float)(m.m[0] - 1.0), (float)m.m[1],
                                (float)m.m[5], (float)m.m[3], (float)(m.m[4] - 1.0)};
            for (int e = 0; e < 6; ++e) ok = ok && std::isfinite(r[e]);
            if (ok)
                for (int e = 0; e < 6; ++e) q[e] = r[e];
        }
        for (int e = 0; e < 6; ++e) corrections[6 * (size_t)k + e] = q[e];
        if (status) status[k] = ok ? 1 : 0;
    }
    if (replaced) *replaced = bad;
    return DIS_OK;
}
