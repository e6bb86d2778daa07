// THE DISTORTION RULE of include/ls2fm.h and its Jacobian, stated once for the two kernels of csrc/undistort.hip: the image kernel
// runs it in fp32 per output pixel, the key-point kernel in fp64 per point.  Every operation is spelled with a rounded-operation
// intrinsic and the functions are compiled with contraction off, so the result does not depend on the build's -ffp-contract flag.
#pragma once

#include "ls2fm_device.h"

namespace camera_model {

// the rounded operations of the rule in both precisions
__device__ __forceinline__ float add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float sub(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ float mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float quot(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ double add(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double sub(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ double mul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double quot(double a, double b) { return __ddiv_rn(a, b); }

// the LS2FM_CAMERA_PARAMS words of one camera.  Where the view index is uniform over the wave these are scalar loads.
template <class T>
struct Camera {
    T fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6;
};

template <class T>
__device__ __forceinline__ Camera<T> load_camera(const T* __restrict__ cam, int64_t view) {
    const T* q = cam + view * LS2FM_CAMERA_PARAMS;
    return {q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9], q[10], q[11]};
}

// what the rule and its Jacobian share
template <class T>
struct Radial {
    T r2, den, rad;
};

// (x, y) -> (xd, yd): the rule up to the focal lengths
template <class T>
__device__ __forceinline__ Radial<T> distort(const Camera<T>& c, T x, T y, T& xd, T& yd) {
#pragma clang fp contract(off)
    const T one = (T)1, two = (T)2;
    Radial<T> o;
    o.r2 = add(mul(x, x), mul(y, y));
    const T num = add(one, mul(o.r2, add(c.k1, mul(o.r2, add(c.k2, mul(o.r2, c.k3))))));
    o.den = add(one, mul(o.r2, add(c.k4, mul(o.r2, add(c.k5, mul(o.r2, c.k6))))));
    o.rad = quot(num, o.den);
    const T xy = mul(x, y);
    xd = add(mul(x, o.rad), add(mul(mul(two, c.p1), xy), mul(c.p2, add(o.r2, mul(mul(two, x), x)))));
    yd = add(mul(y, o.rad), add(mul(c.p1, add(o.r2, mul(mul(two, y), y))), mul(mul(two, c.p2), xy)));
    return o;
}

// normalised distorted point -> the photograph
template <class T>
__device__ __forceinline__ void to_image(const Camera<T>& c, T xd, T yd, T& u, T& v) {
#pragma clang fp contract(off)
    u = add(mul(c.fx, xd), c.cx);
    v = add(mul(c.fy, yd), c.cy);
}

// J = d(xd, yd)/d(x, y) = [a b; c d] at the point whose Radial is o
template <class T>
__device__ __forceinline__ void jacobian(const Camera<T>& c, const Radial<T>& o, T x, T y, T& ja, T& jb, T& jc, T& jd) {
#pragma clang fp contract(off)
    const T two = (T)2, three = (T)3, six = (T)6;
    const T dnum = add(c.k1, mul(o.r2, add(mul(two, c.k2), mul(o.r2, mul(three, c.k3)))));
    const T dden = add(c.k4, mul(o.r2, add(mul(two, c.k5), mul(o.r2, mul(three, c.k6)))));
    const T g = quot(sub(dnum, mul(o.rad, dden)), o.den);
    const T x2 = mul(two, x), y2 = mul(two, y);
    const T gx = mul(x2, g), gy = mul(y2, g);
    const T p1_2 = mul(two, c.p1), p2_2 = mul(two, c.p2);
    ja = add(add(add(o.rad, mul(x, gx)), mul(p1_2, y)), mul(c.p2, mul(six, x)));
    jb = add(add(mul(x, gy), mul(p1_2, x)), mul(c.p2, y2));
    jc = add(add(mul(y, gx), mul(c.p1, x2)), mul(p2_2, y));
    jd = add(add(add(o.rad, mul(y, gy)), mul(c.p1, mul(six, y))), mul(p2_2, x));
}

// J_k = d(fx xd + cx, fy yd + cy)/d(the 12 words) at the point whose Radial is o and whose distorted point is (xd, yd): row u into
// ju, row v into jv, the words in the camera's order (THE CAMERA BLOCK of include/ls2fm.h)
template <class T>
__device__ __forceinline__ void jacobian_k(const Camera<T>& c, const Radial<T>& o, T x, T y, T xd, T yd, T (&ju)[12], T (&jv)[12]) {
#pragma clang fp contract(off)
    const T zero = (T)0, one = (T)1, two = (T)2;
    const T fxx = mul(c.fx, x), fyy = mul(c.fy, y), xy2 = mul(two, mul(x, y));
    const T q1 = quot(o.r2, o.den), q2 = mul(q1, o.r2), q3 = mul(q2, o.r2);                 // r2^j / den
    const T n1 = sub(zero, mul(o.rad, q1)), n2 = sub(zero, mul(o.rad, q2)), n3 = sub(zero, mul(o.rad, q3));
    ju[0] = xd;   jv[0] = zero;
    ju[1] = zero; jv[1] = yd;
    ju[2] = one;  jv[2] = zero;
    ju[3] = zero; jv[3] = one;
    ju[4] = mul(fxx, q1); jv[4] = mul(fyy, q1);
    ju[5] = mul(fxx, q2); jv[5] = mul(fyy, q2);
    ju[6] = mul(c.fx, xy2); jv[6] = mul(c.fy, add(o.r2, mul(mul(two, y), y)));
    ju[7] = mul(c.fx, add(o.r2, mul(mul(two, x), x))); jv[7] = mul(c.fy, xy2);
    ju[8] = mul(fxx, q3); jv[8] = mul(fyy, q3);
    ju[9] = mul(fxx, n1); jv[9] = mul(fyy, n1);
    ju[10] = mul(fxx, n2); jv[10] = mul(fyy, n2);
    ju[11] = mul(fxx, n3); jv[11] = mul(fyy, n3);
}

}  // namespace camera_model
