// pose_host.h — the small host pose helpers of the entries in front of the solver, as Eigen / Sophus
// evaluate them: one rounding per operation (contraction off whatever the including file's flags are),
// every expression in the order written.
#pragma once

namespace deftri {

// Eigen's Quaternion::toRotationMatrix of (x y z w): row-major R [9]
template <typename T> inline void quat_to_rotation(const T *q, T *R) {
#pragma clang fp contract(off)
    const T x = q[0], y = q[1], z = q[2], w = q[3];
    const T tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w;
    const T txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
    R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}

// poses row-major 3x4 [R | t].  Sophus' inverse(): [R^T | -(R^T t)]
inline void pose34_inverse(const float *T, float *Ti) {
#pragma clang fp contract(off)
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Ti[4 * i + j] = T[4 * j + i];
    for (int i = 0; i < 3; i++) Ti[4 * i + 3] = -(Ti[4 * i] * T[3] + Ti[4 * i + 1] * T[7] + Ti[4 * i + 2] * T[11]);
}

// AB = A * B: [Ra Rb | Ra tb + ta]
inline void pose34_product(const float *A, const float *B, float *AB) {
#pragma clang fp contract(off)
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) AB[4 * i + j] = A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j] + A[4 * i + 2] * B[8 + j];
        AB[4 * i + 3] = (A[4 * i] * B[3] + A[4 * i + 1] * B[7] + A[4 * i + 2] * B[11]) + A[4 * i + 3];
    }
}

}  // namespace deftri
