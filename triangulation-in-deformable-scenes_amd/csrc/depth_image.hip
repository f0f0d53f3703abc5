// depth_image.hip — the real-image input path: the keyframes' depth images resident on the context,
// KeyFrame::getDepthMeasure on the device (k_depth_sample, device_math.h's depth_measure_px; the same
// function on the host for a host-only context), the per-keyframe sample cache the graph builds read,
// and measureRealAbsoluteMapErrors (Measurements.cc:101-348): per matched slot the fp32 terms on the
// device (k_real_abs_terms, k_real_abs_scaled_terms), summed in fp64 in measurements.hip's fixed
// order (no atomics), the totals cast to float before the reference's float divisions.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/deftri.h"
#include "depth_image.h"
#include "dev_arena.h"
#include "device_math.h"
#include "kernels.h"
#include "measure_scratch.h"
#include "pose_host.h"

namespace deftri {
namespace dev {

#define TID (blockIdx.x * blockDim.x + threadIdx.x)

// one thread per pixel; the status is decided before any load (depth_measure_px)
__global__ void k_depth_sample(int n, const float *__restrict__ img, int rows, int cols, double scale,
                               const float *__restrict__ uv, int scaled, double *__restrict__ depth,
                               unsigned char *__restrict__ status) {
    const int k = TID;
    if (k >= n) return;
    unsigned char st;
    depth[k] = depth_measure_px(img, rows, cols, scale, uv[2 * k], uv[2 * k + 1], scaled, &st);
    status[k] = st;
}

// fp32, one rounding per operation, as the reference's Eigen expressions
#pragma clang fp contract(off)
// x3D = (PinHole::unproject(x) / z) * d, then T.inverse().matrix() * [x3D; 1] (Eigen's 4x4 * 4x1,
// column by column).  The float vector times the double scalar: the scalar is cast to float first
// (Eigen's scalar promotion).  ti: rows of R_inv (9) and t_inv (3)
__device__ __forceinline__ void real_abs_world(const float *ph, const float *ti, const float *uv, float d, float x3[3],
                                               float w[3]) {
    float m[3] = {(uv[0] - ph[2]) / ph[0], (uv[1] - ph[3]) / ph[1], 1.0f};
    const float z = m[2];
    m[0] /= z; m[1] /= z; m[2] /= z;
    x3[0] = m[0] * d; x3[1] = m[1] * d; x3[2] = m[2] * d;
#pragma unroll
    for (int r = 0; r < 3; r++) w[r] = ((ti[3 * r] * x3[0] + ti[3 * r + 1] * x3[1]) + ti[3 * r + 2] * x3[2]) + ti[9 + r];
}
__device__ __forceinline__ float sqn3(const float v[3]) { return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]; }

// pass 1 of a pair (:149-246), per matched slot k.  in: uv [4k] (x1, x2), d [2k] (d1, d2), p [6k] (the
// MapPoints' positions), cams: ph (4), T1w^-1 (12), T2w^-1 (12), then q1 (4) t1 (3) q2 (4) t2 (3) of
// T1w / T2w.  out (n each): movement, original error, moved error, their squares (2), x3D1.z / (T1w
// p1).z, x3D2.z / (T2w p2).z
__global__ void k_real_abs_terms(int n, const float *__restrict__ uv, const double *__restrict__ d,
                                 const float *__restrict__ p, const float *__restrict__ cams, double *__restrict__ out) {
    const int k = TID;
    if (k >= n) return;
    float x1[3], x2[3], w1[3], w2[3];
    real_abs_world(cams, cams + 4, uv + 4 * (size_t)k, (float)d[2 * k], x1, w1);
    real_abs_world(cams, cams + 16, uv + 4 * (size_t)k + 2, (float)d[2 * k + 1], x2, w2);
    const float *p1 = p + 6 * (size_t)k, *p2 = p1 + 3;
    float z[2];
#pragma unroll
    for (int c = 0; c < 2; c++) {
        // (T * p).z: the unit quaternion's _transformVector, then + t
        const float *q = cams + 28 + 7 * c, *v = c ? p2 : p1;
        float a[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
        a[0] += a[0]; a[1] += a[1]; a[2] += a[2];
        const float cz = q[0] * a[1] - q[1] * a[0];
        z[c] = ((v[2] + q[3] * a[2]) + cz) + q[6];
    }
    float mv[3], e1[3], e2[3];
#pragma unroll
    for (int r = 0; r < 3; r++) { mv[r] = w1[r] - w2[r]; e1[r] = p1[r] - w1[r]; e2[r] = p2[r] - w2[r]; }
    const float s1 = sqn3(e1), s2 = sqn3(e2);
    out[k] = (double)sqrtf(sqn3(mv));
    out[(size_t)n + k] = (double)sqrtf(s1);
    out[2 * (size_t)n + k] = (double)sqrtf(s2);
    out[3 * (size_t)n + k] = (double)s1;
    out[4 * (size_t)n + k] = (double)s2;
    out[5 * (size_t)n + k] = (double)(x1[2] / z[0]);
    out[6 * (size_t)n + k] = (double)(x2[2] / z[1]);
}

// pass 2 (:250-309): x3D = m * d / scale (the product first, then the float division); out (n each):
// the up-to-scale original and moved error
__global__ void k_real_abs_scaled_terms(int n, const float *__restrict__ uv, const double *__restrict__ d,
                                        const float *__restrict__ p, const float *__restrict__ cams, float scale1,
                                        float scale2, double *__restrict__ out) {
    const int k = TID;
    if (k >= n) return;
    float e[2];
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const float *u = uv + 4 * (size_t)k + 2 * c, *ph = cams, *ti = cams + 4 + 12 * c;
        const float dd = (float)d[2 * k + c], sc = c ? scale2 : scale1;
        float m[3] = {(u[0] - ph[2]) / ph[0], (u[1] - ph[3]) / ph[1], 1.0f};
        const float z = m[2];
        m[0] /= z; m[1] /= z; m[2] /= z;
        const float x3[3] = {m[0] * dd / sc, m[1] * dd / sc, m[2] * dd / sc};
        const float *pp = p + 6 * (size_t)k + 3 * c;
        float er[3];
#pragma unroll
        for (int r = 0; r < 3; r++)
            er[r] = pp[r] - (((ti[3 * r] * x3[0] + ti[3 * r + 1] * x3[1]) + ti[3 * r + 2] * x3[2]) + ti[9 + r]);
        e[c] = sqrtf(sqn3(er));
    }
    out[k] = (double)e[0];
    out[(size_t)n + k] = (double)e[1];
}
#pragma clang fp contract(on)

}  // namespace dev

// ---- the images of a context ------------------------------------------------------------------

void DepthImages::clear() {
    if (dev_ >= 0 && !imgs_.empty()) hipSetDevice(dev_);
    for (Image &im : imgs_)
        if (im.dev) hipFree(im.dev);
    imgs_.clear();
}

DepthImages::Image *DepthImages::find(int64_t kf_id) {
    for (Image &im : imgs_)
        if (im.kf_id == kf_id) return &im;
    return nullptr;
}

bool DepthImages::device_image(int64_t kf_id, const float **pixels, int32_t *rows, int32_t *cols, double *scale) {
    Image *im = find(kf_id);
    if (!im || !im->dev) return false;
    *pixels = im->dev; *rows = im->rows; *cols = im->cols; *scale = im->scale;
    return true;
}

int DepthImages::set(int32_t n, const deftri_depth_image *images, std::string &err) {
    if (n < 0 || (n > 0 && !images)) { err = "bad depth image list"; return DEFTRI_E_ARG; }
    for (int32_t i = 0; i < n; i++) {
        const deftri_depth_image &d = images[i];
        if (d.rows <= 0 || d.cols <= 0 || !d.pixels || (int64_t)d.rows * d.cols > (int64_t)1 << 30) {
            err = "bad depth image: keyframe " + std::to_string(d.kf_id);
            return DEFTRI_E_ARG;
        }
        for (int32_t j = 0; j < i; j++)
            if (images[j].kf_id == d.kf_id) { err = "two depth images for keyframe " + std::to_string(d.kf_id); return DEFTRI_E_ARG; }
    }
    clear();
    imgs_.resize((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        const deftri_depth_image &d = images[i];
        Image &im = imgs_[i];
        im.kf_id = d.kf_id; im.rows = d.rows; im.cols = d.cols; im.scale = d.image_depth_scale;
        std::memcpy(im.ph, d.ph, sizeof(im.ph));
        const size_t np = (size_t)d.rows * d.cols;
        if (dev_ < 0) {
            im.host.assign(d.pixels, d.pixels + np);
        } else {
            if (hipSetDevice(dev_) != hipSuccess || hipMalloc((void **)&im.dev, sizeof(float) * np) != hipSuccess ||
                hipMemcpy(im.dev, d.pixels, sizeof(float) * np, hipMemcpyHostToDevice) != hipSuccess) {
                clear();
                err = "depth image upload failed";
                return DEFTRI_E_HIP;
            }
        }
        uploads++;
    }
    return 0;
}

int DepthImages::sample(Image &im, int32_t n, const float *uv, int scaled, double *depth, uint8_t *status, std::string &err) {
    if (n == 0) return 0;
    if (dev_ < 0) {
        for (int32_t k = 0; k < n; k++)
            depth[k] = dev::depth_measure_px(im.host.data(), im.rows, im.cols, im.scale, uv[2 * k], uv[2 * k + 1], scaled,
                                             &status[k]);
        return 0;
    }
    if (hipSetDevice(dev_) != hipSuccess) { err = "hipSetDevice"; return DEFTRI_E_HIP; }
    DevArena A;
    float *d_uv;
    double *d_depth;
    uint8_t *d_st;
    A.add(&d_uv, 2 * (size_t)n); A.add(&d_depth, (size_t)n); A.add(&d_st, (size_t)n);
    if (!A.commit()) { err = "depth sampling: allocation failed"; return DEFTRI_E_HIP; }
    hipMemcpy(d_uv, uv, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(dev::k_depth_sample, dim3(nblk(n, 256)), dim3(256), 0, st_, (int)n, im.dev, im.rows, im.cols, im.scale,
                       d_uv, scaled, d_depth, d_st);
    if (hipMemcpyAsync(depth, d_depth, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st_) != hipSuccess ||
        hipMemcpyAsync(status, d_st, (size_t)n, hipMemcpyDeviceToHost, st_) != hipSuccess ||
        hipStreamSynchronize(st_) != hipSuccess) {
        err = std::string("depth sampling: ") + hipGetErrorString(hipGetLastError());
        return DEFTRI_E_HIP;
    }
    return 0;
}

int DepthImages::measure(int64_t kf_id, int32_t n, const float *uv, int scaled, double *depth, uint8_t *status,
                         std::string &err) {
    if (n < 0 || (n > 0 && !uv)) { err = "bad pixel list"; return DEFTRI_E_ARG; }
    Image *im = find(kf_id);
    if (!im) { err = "Depth image is not initialized: keyframe " + std::to_string(kf_id); return DEFTRI_E_ARG; }
    std::vector<double> d(depth ? 0 : (size_t)n);
    std::vector<uint8_t> s(status ? 0 : (size_t)n);
    return sample(*im, n, uv, scaled ? 1 : 0, depth ? depth : d.data(), status ? status : s.data(), err);
}

int DepthImages::views(const deftri_map &map, std::vector<DepthView> &out, std::string &err) {
    out.assign((size_t)std::max(map.n_keyframes, 0), DepthView());
    for (int a = 0; a < map.n_keyframes; a++) {
        const deftri_keyframe &kf = map.keyframes[a];
        Image *im = find(kf.id);
        if (!im) continue;
        if (kf.n_obs < 0 || (kf.n_obs > 0 && !kf.kp_uv)) { err = "bad map: keyframe arrays"; return DEFTRI_E_ARG; }
        const size_t no = (size_t)kf.n_obs;
        if (!im->cached || im->uv.size() != 2 * no || (no && std::memcmp(im->uv.data(), kf.kp_uv, 8 * no) != 0)) {
            im->cached = false;
            im->uv.assign(kf.kp_uv, kf.kp_uv + 2 * no);
            im->raw.assign(no, 0.0); im->meas.assign(no, 0.0); im->status.assign(no, 0);
            const int rc = sample(*im, (int32_t)no, im->uv.data(), 1, im->raw.data(), im->status.data(), err);
            if (rc) return rc;
            // getDepthMeasure(.., false) = depth * imageDepthScale_: one double product of the sampled value
            for (size_t o = 0; o < no; o++) im->meas[o] = im->raw[o] * im->scale;
            im->cached = true;
            samplings++;
        }
        out[a].raw = im->raw.data(); out[a].meas = im->meas.data(); out[a].status = im->status.data(); out[a].ph = im->ph;
    }
    return 0;
}

std::string depth_status_message(int64_t kf_id, int32_t obs, const float *uv, int status) {
    char buf[200];
    std::snprintf(buf, sizeof(buf), "keyframe %lld observation %d: pixel (%g, %g) %s", (long long)kf_id, (int)obs, (double)uv[0],
                  (double)uv[1], status == 1 ? "is out of range of the depth image" : "reads outside the depth image");
    return buf;
}

// ---- measureRealAbsoluteMapErrors --------------------------------------------------------------

namespace {
#pragma clang fp contract(off)
// Sophus::SE3f::inverse().matrix(): the conjugate quaternion's rotation matrix (Eigen toRotationMatrix,
// float) and invR * (-t) by the quaternion-vector product; rows of R (9), t (3)
void se3f_inverse_rows(const float q[4], const float t[3], float out[12]) {
    const float x = -q[0], y = -q[1], z = -q[2], w = q[3];
    const float conj[4] = {x, y, z, w};
    quat_to_rotation(conj, out);
    const float v[3] = {-t[0], -t[1], -t[2]};
    float uv[3] = {y * v[2] - z * v[1], z * v[0] - x * v[2], x * v[1] - y * v[0]};
    for (float &u : uv) u += u;
    const float c[3] = {y * uv[2] - z * uv[1], z * uv[0] - x * uv[2], x * uv[1] - y * uv[0]};
    for (int k = 0; k < 3; k++) out[9 + k] = (v[k] + w * uv[k]) + c[k];
}
#pragma clang fp contract(on)
}  // namespace

int measure_real_absolute(DepthImages &di, int device, hipStream_t st, const deftri_map &map, deftri_real_abs_errors *out,
                          std::string &err) {
    std::memset(out, 0, sizeof(*out));
    const int K = map.n_keyframes;
    if (K < 0 || (K > 0 && !map.keyframes)) { err = "bad map"; return DEFTRI_E_ARG; }
    for (int a = 0; a < K; a++) {
        const deftri_keyframe &f = map.keyframes[a];
        if (f.n_slots < 0 || f.n_obs < 0 || (f.n_slots > 0 && (!f.point_id || !f.point_pos || !f.obs_index)) ||
            (f.n_obs > 0 && !f.kp_uv)) { err = "bad map: keyframe arrays"; return DEFTRI_E_ARG; }
    }
    // Map::getMapPoints(): the distinct MapPoint ids the keyframes' slots hold
    std::vector<int64_t> ids;
    for (int a = 0; a < K; a++)
        for (int s = 0; s < map.keyframes[a].n_slots; s++)
            if (map.keyframes[a].point_id[s] >= 0) ids.push_back(map.keyframes[a].point_id[s]);
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    const int64_t point_count = (int64_t)ids.size();
    out->point_count = point_count;
    std::vector<DepthView> dv;
    int rc = di.views(map, dv, err);
    if (rc) return rc;
    if (hipSetDevice(device) != hipSuccess) return DEFTRI_E_NODEVICE;
    // the reference's float accumulators, fed by the fp64 fixed-order sums of each pair's terms
    double tot[5] = {0, 0, 0, 0, 0}, up[2] = {0, 0};
    float scale1 = 0, scale2 = 0;
    int64_t n_points = 0;
    for (int a = 0; a < K; a++)
        for (int b = a + 1; b < K; b++) {
            const deftri_keyframe &kf1 = map.keyframes[b], &kf2 = map.keyframes[a];    // camera 1 = k2
            if (!dv[b].raw || !dv[a].raw) {
                err = "Depth image is not initialized: keyframe " + std::to_string(!dv[b].raw ? kf1.id : kf2.id);
                return DEFTRI_E_ARG;
            }
            if (kf2.n_slots < kf1.n_slots) { err = "keyframe 2 has fewer slots than keyframe 1"; return DEFTRI_E_ARG; }
            std::vector<float> uv, pw;
            std::vector<double> d;
            for (int i = 0; i < kf1.n_slots; i++) {
                if (kf1.point_id[i] < 0 || kf2.point_id[i] < 0) continue;
                const int32_t o1 = kf1.obs_index[i], o2 = kf2.obs_index[i];
                if (o1 < 0 || o2 < 0) continue;
                if (o1 >= kf1.n_obs || o2 >= kf2.n_obs) { err = "observation index out of range"; return DEFTRI_E_ARG; }
                if (dv[b].status[o1]) { err = depth_status_message(kf1.id, o1, kf1.kp_uv + 2 * (size_t)o1, dv[b].status[o1]); return DEFTRI_E_ARG; }
                if (dv[a].status[o2]) { err = depth_status_message(kf2.id, o2, kf2.kp_uv + 2 * (size_t)o2, dv[a].status[o2]); return DEFTRI_E_ARG; }
                uv.push_back(kf1.kp_uv[2 * (size_t)o1]); uv.push_back(kf1.kp_uv[2 * (size_t)o1 + 1]);
                uv.push_back(kf2.kp_uv[2 * (size_t)o2]); uv.push_back(kf2.kp_uv[2 * (size_t)o2 + 1]);
                d.push_back(dv[b].raw[o1]); d.push_back(dv[a].raw[o2]);      // getDepthMeasure(x, y): scaled
                for (int c = 0; c < 3; c++) pw.push_back(kf1.point_pos[3 * (size_t)i + c]);
                for (int c = 0; c < 3; c++) pw.push_back(kf2.point_pos[3 * (size_t)i + c]);
            }
            const int64_t n = (int64_t)d.size() / 2;
            // both pixels are unprojected with keyframe 1's pinhole calibration (:145,193,197)
            std::vector<float> cams(42);
            for (int c = 0; c < 4; c++) cams[c] = dv[b].ph[c];
            const deftri_keyframe *ks[2] = {&kf1, &kf2};
            for (int c = 0; c < 2; c++) {
                float q[4], t[3];
                for (int i = 0; i < 4; i++) q[i] = (float)ks[c]->pose[i];
                for (int i = 0; i < 3; i++) t[i] = (float)ks[c]->pose[4 + i];
                se3f_inverse_rows(q, t, &cams[4 + 12 * c]);
                for (int i = 0; i < 4; i++) cams[28 + 7 * c + i] = q[i];
                for (int i = 0; i < 3; i++) cams[28 + 7 * c + 4 + i] = t[i];
            }
            n_points += n;
            DevArena A;
            float *d_uv, *d_pw, *d_cams;
            double *d_d, *terms, *part, *dout;
            A.add(&d_uv, uv.size()); A.add(&d_pw, pw.size()); A.add(&d_cams, cams.size()); A.add(&d_d, d.size());
            A.add(&terms, 7 * (size_t)n); A.add(&part, 256); A.add(&dout, 8);
            if (!A.commit()) { err = "allocation failed"; return DEFTRI_E_HIP; }
            upload(d_uv, uv); upload(d_pw, pw); upload(d_cams, cams); upload(d_d, d);
            double s[7] = {0, 0, 0, 0, 0, 0, 0};
            if (n > 0) {
                hipLaunchKernelGGL(dev::k_real_abs_terms, dim3(nblk(n, 256)), dim3(256), 0, st, (int)n, d_uv, d_d, d_pw, d_cams, terms);
                if (sums(terms, n, 7, part, dout, s, st)) { err = "real absolute errors: device sums failed"; return DEFTRI_E_HIP; }
            }
            for (int c = 0; c < 5; c++) tot[c] += s[c];
            // scale += ...; scale = scale / n_points (:215-216,247-248): the float accumulators carry across
            // the pairs; n_points == 0 divides by zero as the reference (NaN scales)
            scale1 = (float)((double)scale1 + s[5]);
            scale2 = (float)((double)scale2 + s[6]);
            scale1 = scale1 / (float)n_points;
            scale2 = scale2 / (float)n_points;
            double s2[2] = {0, 0};
            if (n > 0) {
                hipLaunchKernelGGL(dev::k_real_abs_scaled_terms, dim3(nblk(n, 256)), dim3(256), 0, st, (int)n, d_uv, d_d, d_pw,
                                   d_cams, scale1, scale2, terms);
                if (sums(terms, n, 2, part, dout, s2, st)) { err = "real absolute errors: device sums failed"; return DEFTRI_E_HIP; }
            }
            up[0] += s2[0]; up[1] += s2[1];
        }
    out->n_points = n_points;
    out->scale1 = (double)scale1;
    out->scale2 = (double)scale2;
    if (point_count > 0) {
        const int in_kf = (int)(point_count / 2.0);
        const float tm = (float)tot[0], te = (float)(tot[1] + tot[2]), tsq = (float)(tot[3] + tot[4]);
        const float tup = (float)(up[0] + up[1]);
        out->average_movement = (double)(tm / in_kf) * 1000;
        out->average_error = (double)(te / (float)point_count) * 1000;
        out->rmse = (double)std::sqrt(tsq / (float)point_count) * 1000;
        out->average_up_to_scale_error = (double)(tup / (float)point_count) * 1000;
    }
    return 0;
}

}  // namespace deftri
