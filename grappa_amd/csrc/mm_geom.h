// Internal coordinates of the molecular-mechanics terms and their derivatives (fp32), shared by csrc/mm_energy.hip (energy, gradient
// and backward over a batch) and csrc/relax.hip (the fused minimiser): ONE definition of the geometry, its guards and the torsion series.
// Geometry follows models/internal_coordinates.py:150-210 (distance, atan2 angle, timemachine dihedral) without the reference's random
// dihedral noise.
#pragma once
#include "common.h"

namespace {

struct V3 {
    float x, y, z;
};
__device__ inline V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ inline V3 operator*(float s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ inline float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ inline V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ inline V3 ldv(const float* __restrict__ p, int atom, int C, int c) {
    const float* q = p + ((size_t)atom * C + c) * 3;
    return {q[0], q[1], q[2]};
}
constexpr float TINY = 1e-20f;

// bond: r = |x0 - x1| ; dr/dx0 = u, dr/dx1 = -u
__device__ inline float bond_geom(V3 p0, V3 p1, V3& u) {
    const V3 d = p0 - p1;
    const float r = sqrtf(dot(d, d));
    u = (1.0f / fmaxf(r, TINY)) * d;
    return r;
}
// angle at p1: theta = atan2(|u x v|, u.v), u = p0-p1, v = p2-p1 ; e0 = dtheta/dp0, e2 = dtheta/dp2, dtheta/dp1 = -(e0+e2)
__device__ inline float angle_geom(V3 p0, V3 p1, V3 p2, V3& e0, V3& e2) {
    const V3 u = p0 - p1, v = p2 - p1;
    const V3 w = cross(u, v);
    const float wl = sqrtf(dot(w, w));
    const float theta = atan2f(wl, dot(u, v));
    const float iw = 1.0f / fmaxf(wl, TINY);
    e0 = (iw / fmaxf(dot(u, u), TINY)) * cross(u, w);
    e2 = (iw / fmaxf(dot(v, v), TINY)) * cross(w, v);
    return theta;
}
// dihedral (reference convention): a = p1-p0, b = p1-p2, c = p3-p2, n1 = a x b, n2 = b x c,
// phi = atan2((n1 x n2).b/|b|, n1.n2);  d0 = -|b| n1/|n1|^2, d3 = |b| n2/|n2|^2,
// d1 = (p-1) d0 - q d3, d2 = (q-1) d3 - p d0 with p = a.b/|b|^2, q = c.b/|b|^2
__device__ inline float dihedral_geom(V3 p0, V3 p1, V3 p2, V3 p3, V3& d0, V3& d1, V3& d2, V3& d3) {
    const V3 a = p1 - p0, b = p1 - p2, c = p3 - p2;
    const V3 n1 = cross(a, b), n2 = cross(b, c);
    const float b2 = dot(b, b);
    const float bl = sqrtf(b2);
    const float y = dot(cross(n1, n2), b) / fmaxf(bl, TINY);
    const float x = dot(n1, n2);
    const float phi = atan2f(y, x);
    d0 = (-bl / fmaxf(dot(n1, n1), TINY)) * n1;
    d3 = (bl / fmaxf(dot(n2, n2), TINY)) * n2;
    const float ib2 = 1.0f / fmaxf(b2, TINY);
    const float p = dot(a, b) * ib2, q = dot(c, b) * ib2;
    d1 = (p - 1.0f) * d0 - q * d3;
    d2 = (q - 1.0f) * d3 - p * d0;
    return phi;
}

__device__ inline float torsion_energy(const float* __restrict__ k, int n_per, float phi, int offset) {
    float e = 0.f;
    for (int n = 1; n <= n_per; ++n) {
        const float kn = k[n - 1];
        e += kn * cosf((float)n * phi);
        if (offset) e += fabsf(kn);
    }
    return e;
}

// d/dphi of sum_n k_n cos(n phi)
__device__ inline float torsion_dcoef(const float* __restrict__ k, int n_per, float phi) {
    float coef = 0.f;
    for (int n = 1; n <= n_per; ++n) coef -= (float)n * k[n - 1] * sinf((float)n * phi);
    return coef;
}

}  // namespace
