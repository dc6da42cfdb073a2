// Internal coordinates of the molecular-mechanics terms and their derivatives (fp32), shared by csrc/mm_energy.hip (energy, gradient
// and backward over a batch), csrc/rx_force.h (the fused minimiser and dynamics) and csrc/relax_steps.hip: ONE definition of the
// geometry, its guards, the torsion series, the bonded gather of an atom and the energy of a tuple.
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

// The bonded gradient of one atom over its incidences q = first, first + stride, .. < last (inc_code[q] = tuple << 4 | level << 2 | position
// of the atom in the tuple): coefficient times d(internal coordinate)/dx in closed form.  ld maps an atom index to its coordinates.
template <class Ld>
__device__ inline V3 bonded_gather(const grappa_mm_desc& d, int first, int last, int stride, Ld ld) {
    V3 g = {0.f, 0.f, 0.f};
    for (int q = first; q < last; q += stride) {
        const int code = d.inc_code[q];
        const int pos = code & 3, l = (code >> 2) & 3, t = code >> 4;
        if (l == 0) {
            V3 u;
            const float r = bond_geom(ld(d.idx[0][2 * t]), ld(d.idx[0][2 * t + 1]), u);
            const float coef = d.k[0][t] * (r - d.eq[0][t]);
            g = g + (pos == 0 ? coef : -coef) * u;
        } else if (l == 1) {
            V3 e0, e2;
            const float th = angle_geom(ld(d.idx[1][3 * t]), ld(d.idx[1][3 * t + 1]), ld(d.idx[1][3 * t + 2]), e0, e2);
            const float coef = d.k[1][t] * (th - d.eq[1][t]);
            const V3 dv = pos == 0 ? e0 : (pos == 2 ? e2 : (-1.0f) * (e0 + e2));
            g = g + coef * dv;
        } else {
            V3 d0, d1, d2, d3;
            const int* id = d.idx[l] + 4 * (size_t)t;
            const float phi = dihedral_geom(ld(id[0]), ld(id[1]), ld(id[2]), ld(id[3]), d0, d1, d2, d3);
            const float coef = torsion_dcoef(d.k[l] + (size_t)t * d.n_per[l], d.n_per[l], phi);
            const V3 dv = pos == 0 ? d0 : (pos == 1 ? d1 : (pos == 2 ? d2 : d3));
            g = g + coef * dv;
        }
    }
    return g;
}

// The energy of tuple t of level l (0 bond, 1 angle, 2 proper, 3 improper); x: its internal coordinate.  ld as for bonded_gather.
template <class Ld>
__device__ inline float bonded_tuple_energy(const grappa_mm_desc& d, int l, int t, Ld ld, float& x) {
    if (l == 0) {
        V3 u;
        x = bond_geom(ld(d.idx[0][2 * t]), ld(d.idx[0][2 * t + 1]), u);
        const float dx = x - d.eq[0][t];
        return 0.5f * d.k[0][t] * dx * dx;
    }
    if (l == 1) {
        V3 e0, e2;
        x = angle_geom(ld(d.idx[1][3 * t]), ld(d.idx[1][3 * t + 1]), ld(d.idx[1][3 * t + 2]), e0, e2);
        const float dx = x - d.eq[1][t];
        return 0.5f * d.k[1][t] * dx * dx;
    }
    V3 d0, d1, d2, d3;
    const int* id = d.idx[l] + 4 * (size_t)t;
    x = dihedral_geom(ld(id[0]), ld(id[1]), ld(id[2]), ld(id[3]), d0, d1, d2, d3);
    return torsion_energy(d.k[l] + (size_t)t * d.n_per[l], d.n_per[l], x, d.offset_torsion);
}

}  // namespace
