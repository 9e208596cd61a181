// srl_consensus_math.h -- internal: the per-lane arithmetic of srl_consensus.hip (sampling, the 7-point and P3P minimal solvers, the two
// error functions), written so that it also compiles as plain C++ for a host build: every function is FP64, branches only on its own
// data and touches no memory but its arguments.  The contract of the results is in include/srlivo_hip.h.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SRL_CONS_FN __host__ __device__ inline
#else
#define SRL_CONS_FN inline
#endif

// ------------------------------------------------------------------------------------------------ the counter-based generator
// draw(seed, hypothesis, k, m) in [0, m): z = ((seed << 32) | hypothesis) * 0x9E3779B97F4A7C15 + (k + 1) * 0xBF58476D1CE4E5B9 (mod 2^64),
// mixed by the splitmix64 finaliser (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31), and
// scaled as ((z >> 32) * m) >> 32.  A pure function: nothing is carried from draw to draw, lane to lane or call to call.
SRL_CONS_FN uint32_t cons_draw(uint32_t seed, uint32_t hypothesis, uint32_t k, uint32_t m) {
    uint64_t z = (((uint64_t)seed << 32) | (uint64_t)hypothesis) * 0x9E3779B97F4A7C15ull + (uint64_t)(k + 1u) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (uint32_t)(((z >> 32) * (uint64_t)m) >> 32);
}

#define SRL_CONS_MAX_DRAWS 64
// S distinct positions in [0, m): draws k = 0, 1, ... in turn, one that repeats an earlier position is rejected; false (no sample) when
// m < S or SRL_CONS_MAX_DRAWS draws did not yield S positions
template <int S>
SRL_CONS_FN bool cons_sample(uint32_t seed, uint32_t hypothesis, int m, int *pos) {
    for (int k = 0; k < S; k++) pos[k] = -1;
    if (m < S) return false;
    int got = 0;
    for (uint32_t d = 0; d < SRL_CONS_MAX_DRAWS && got < S; d++) {
        const int c = (int)cons_draw(seed, hypothesis, d, (uint32_t)m);
        bool repeated = false;
        for (int k = 0; k < S; k++) repeated = repeated || pos[k] == c;
        if (repeated) continue;
        for (int k = 0; k < S; k++) if (k == got) pos[k] = c;
        got++;
    }
    return got == S;
}

// ------------------------------------------------------------------------------------------------ the two error functions
// The ORDER below is the contract (include/srlivo_hip.h): + - * / only, no contraction, so that float64 NumPy reproduces every bit.
// Fundamental: F row-major, (x1, y1) the last image's point, (x2, y2) the current one's.
SRL_CONS_FN bool cons_inlier_fundamental(const double *F, double x1, double y1, double x2, double y2, double thr2) {
    const double a = (F[0] * x1 + F[1] * y1) + F[2], b = (F[3] * x1 + F[4] * y1) + F[5], c = (F[6] * x1 + F[7] * y1) + F[8];      // F x1
    const double d2 = (a * x2 + b * y2) + c;
    const double e2 = (d2 * d2) / (a * a + b * b);
    const double at = (F[0] * x2 + F[3] * y2) + F[6], bt = (F[1] * x2 + F[4] * y2) + F[7], ct = (F[2] * x2 + F[5] * y2) + F[8];   // F^T x2
    const double d1 = (at * x1 + bt * y1) + ct;
    const double e1 = (d1 * d1) / (at * at + bt * bt);
    return e1 <= thr2 && e2 <= thr2;               // = max(e1, e2) <= thr2; false for a NaN
}
// PnP: M = R row-major (9) then t (3); K = fx, fy, cx, cy
SRL_CONS_FN bool cons_inlier_pnp(const double *M, const double *K, double X, double Y, double Z, double u, double v, double thr2) {
    const double xc = ((M[0] * X + M[1] * Y) + M[2] * Z) + M[9];
    const double yc = ((M[3] * X + M[4] * Y) + M[5] * Z) + M[10];
    const double zc = ((M[6] * X + M[7] * Y) + M[8] * Z) + M[11];
    const double du = (K[0] * (xc / zc) + K[2]) - u, dv = (K[1] * (yc / zc) + K[3]) - v;
    const double e = du * du + dv * dv;
    return zc > 0.0 && e <= thr2;
}

// ------------------------------------------------------------------------------------------------ real roots of a cubic and a quartic
SRL_CONS_FN double cons_polish(const double *c, int degree, double x) {      // c[0] + c[1] x + ...: three Newton steps
    for (int it = 0; it < 3; it++) {
        double f = c[degree], df = 0.0;
        for (int k = degree - 1; k >= 0; k--) { df = df * x + f; f = f * x + c[k]; }
        const double step = f / df;
        if (!(df != 0.0) || !std::isfinite(step)) break;
        x -= step;
    }
    return x;
}
// Roots come in FIXED slots, an absent one as NaN: nothing is appended at a run-time index, so the slots stay in registers.
#define SRL_CONS_NO_ROOT (std::nan(""))
// the real roots of x^3 + a x^2 + b x + d in closed form into x[0 .. 2], unpolished: no test of the coefficients' scale, whatever they are
SRL_CONS_FN void cons_cubic_monic(double a, double b, double d, double *x) {
    for (int k = 0; k < 3; k++) x[k] = SRL_CONS_NO_ROOT;
    const double Q = (a * a - 3.0 * b) / 9.0, R = (2.0 * a * a * a - 9.0 * a * b + 27.0 * d) / 54.0;
    const double Q3 = Q * Q * Q, R2 = R * R;
    if (R2 < Q3) {
        double q = R / std::sqrt(Q3);
        q = q > 1.0 ? 1.0 : (q < -1.0 ? -1.0 : q);
        const double theta = std::acos(q), m = -2.0 * std::sqrt(Q);
        x[0] = m * std::cos(theta / 3.0) - a / 3.0;
        x[1] = m * std::cos((theta + 6.283185307179586) / 3.0) - a / 3.0;
        x[2] = m * std::cos((theta - 6.283185307179586) / 3.0) - a / 3.0;
    } else {
        const double A = (R < 0.0 ? 1.0 : -1.0) * std::cbrt(std::fabs(R) + std::sqrt(R2 - Q3));
        const double B = A != 0.0 ? Q / A : 0.0;
        x[0] = (A + B) - a / 3.0;
    }
}
// c[0] + c[1] x + c[2] x^2 + c[3] x^3 into r[0 .. 2]; the number of roots, 0 for a non-finite coefficient or a leading coefficient that
// vanishes against the others (the 7-point cubic of a degenerate sample)
SRL_CONS_FN int cons_cubic(const double *c, double *r) {
    for (int k = 0; k < 3; k++) r[k] = SRL_CONS_NO_ROOT;
    if (!(std::isfinite(c[0]) && std::isfinite(c[1]) && std::isfinite(c[2]) && std::isfinite(c[3]))) return 0;
    if (!(std::fabs(c[3]) > 1e-14 * (std::fabs(c[2]) + std::fabs(c[1]) + std::fabs(c[0])))) return 0;
    double x[3];
    cons_cubic_monic(c[2] / c[3], c[1] / c[3], c[0] / c[3], x);
    int kept = 0;
    for (int k = 0; k < 3; k++) {
        const double p = std::isfinite(x[k]) ? cons_polish(c, 3, x[k]) : SRL_CONS_NO_ROOT;
        r[k] = std::isfinite(p) ? p : SRL_CONS_NO_ROOT;
        kept += std::isfinite(p) ? 1 : 0;
    }
    return kept;
}
// c[0] + ... + c[4] x^4 by Ferrari's resolvent cubic into r[0 .. 3]; up to 4 real roots, each polished on the quartic itself
SRL_CONS_FN int cons_quartic(const double *c, double *r) {
    for (int k = 0; k < 4; k++) r[k] = SRL_CONS_NO_ROOT;
    if (!(std::isfinite(c[0]) && std::isfinite(c[1]) && std::isfinite(c[2]) && std::isfinite(c[3]) && std::isfinite(c[4]))) return 0;
    if (!(std::fabs(c[4]) > 1e-14 * (std::fabs(c[3]) + std::fabs(c[2]) + std::fabs(c[1]) + std::fabs(c[0])))) return 0;
    const double b3 = c[3] / c[4], b2 = c[2] / c[4], b1 = c[1] / c[4], b0 = c[0] / c[4];
    const double p = b2 - 0.375 * b3 * b3;
    const double q = b1 - 0.5 * b3 * b2 + 0.125 * b3 * b3 * b3;
    const double s = b0 - 0.25 * b3 * b1 + 0.0625 * b3 * b3 * b2 - (3.0 / 256.0) * b3 * b3 * b3 * b3;
    // (y^2 + p/2 + m)^2 = 2 m (y - q / (4 m))^2 where 8 m^3 + 8 p m^2 + (2 p^2 - 8 s) m - q^2 = 0
    // Its leading coefficient never vanishes, however large q^2 is beside it (roots spread over decades): no test of the scale here.
    const double rc[4] = {-q * q, 2.0 * p * p - 8.0 * s, 8.0 * p, 8.0};
    double mr[3];
    cons_cubic_monic(p, 0.25 * p * p - s, -0.125 * q * q, mr);
    double m = 0.0;
    for (int k = 0; k < 3; k++) {
        const double mk = std::isfinite(mr[k]) ? cons_polish(rc, 3, mr[k]) : SRL_CONS_NO_ROOT;
        if (mk > m) m = mk;
    }
    double y[4] = {SRL_CONS_NO_ROOT, SRL_CONS_NO_ROOT, SRL_CONS_NO_ROOT, SRL_CONS_NO_ROOT};
    if (m > 1e-14 * (std::fabs(p) + 1.0)) {
        const double w = std::sqrt(2.0 * m), t = q / (2.0 * w), h = 0.5 * p + m;
        const double d1 = w * w - 4.0 * (h + t), d2 = w * w - 4.0 * (h - t);
        if (d1 >= 0.0) { const double e = std::sqrt(d1); y[0] = 0.5 * (w + e); y[1] = 0.5 * (w - e); }
        if (d2 >= 0.0) { const double e = std::sqrt(d2); y[2] = 0.5 * (-w + e); y[3] = 0.5 * (-w - e); }
    } else {                                       // q = 0: a quadratic in y^2
        const double disc = p * p - 4.0 * s;
        if (disc >= 0.0) {
            const double e = std::sqrt(disc), z1 = 0.5 * (-p + e), z2 = 0.5 * (-p - e);
            if (z1 >= 0.0) { y[0] = std::sqrt(z1); y[1] = -std::sqrt(z1); }
            if (z2 >= 0.0) { y[2] = std::sqrt(z2); y[3] = -std::sqrt(z2); }
        }
    }
    int kept = 0;
    for (int k = 0; k < 4; k++) {
        const double x = std::isfinite(y[k]) ? cons_polish(c, 4, y[k] - 0.25 * b3) : SRL_CONS_NO_ROOT;
        r[k] = std::isfinite(x) ? x : SRL_CONS_NO_ROOT;
        kept += std::isfinite(x) ? 1 : 0;
    }
    return kept;
}

// ------------------------------------------------------------------------------------------------ the 7-point solver
SRL_CONS_FN double cons_det3(const double *a, const double *b, const double *c) {      // columns a, b, c taken as ROWS of a 3 x 3 (same determinant)
    return a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]);
}
// The 7 x 9 system W (row r, column c at W[(r * 9 + c) * st]) is reduced in place to [I | B] by Gauss-Jordan elimination with complete
// pivoting; the two null vectors go to W[(63 + 9 v + k) * st].  false: rank below 7 (repeated or collinear points).  st lets the lanes
// of a wave interleave their systems in LDS; the column permutation is nine nibbles of one word, so nothing is indexed in registers.
SRL_CONS_FN bool cons_nullspace_7x9(double *W, int st) {
#define CONS_W(r, c) W[((r) * 9 + (c)) * st]
    uint64_t perm = 0x876543210ull;
    double amax = 0.0;
    for (int e = 0; e < 63; e++) { const double v = std::fabs(W[e * st]); if (!(v <= amax)) amax = v; }
    if (!(amax > 0.0) || !std::isfinite(amax)) return false;
    for (int k = 0; k < 7; k++) {
        double best = -1.0;
        int bi = k, bj = k;
        for (int i = k; i < 7; i++)
            for (int j = k; j < 9; j++) { const double v = std::fabs(CONS_W(i, j)); if (v > best) { best = v; bi = i; bj = j; } }
        if (!(best > 1e-11 * amax)) return false;
        if (bi != k) for (int j = 0; j < 9; j++) { const double t = CONS_W(k, j); CONS_W(k, j) = CONS_W(bi, j); CONS_W(bi, j) = t; }
        if (bj != k) {
            for (int i = 0; i < 7; i++) { const double t = CONS_W(i, k); CONS_W(i, k) = CONS_W(i, bj); CONS_W(i, bj) = t; }
            const uint64_t nk = (perm >> (4 * k)) & 15ull, nj = (perm >> (4 * bj)) & 15ull;
            perm = (perm & ~((15ull << (4 * k)) | (15ull << (4 * bj)))) | (nj << (4 * k)) | (nk << (4 * bj));
        }
        const double inv = 1.0 / CONS_W(k, k);
        for (int j = k; j < 9; j++) CONS_W(k, j) *= inv;
        for (int i = 0; i < 7; i++) {
            if (i == k) continue;
            const double f = CONS_W(i, k);
            for (int j = k; j < 9; j++) CONS_W(i, j) -= f * CONS_W(k, j);
        }
    }
    for (int v = 0; v < 2; v++) {
        double *out = W + (63 + 9 * v) * st;
        for (int i = 0; i < 7; i++) out[(int)((perm >> (4 * i)) & 15ull) * st] = -CONS_W(i, 7 + v);
        out[(int)((perm >> (4 * (7 + v))) & 15ull) * st] = 1.0;
        out[(int)((perm >> (4 * (8 - v))) & 15ull) * st] = 0.0;
    }
#undef CONS_W
    return true;
}
// det(a F1 + (1 - a) F2) = det(B + a D), B = F2, D = F1 - F2: the four coefficients by multilinearity in the rows
SRL_CONS_FN void cons_det_cubic(const double *F1, const double *F2, double *c) {
    double D[9];
    for (int k = 0; k < 9; k++) D[k] = F1[k] - F2[k];
    const double *b0 = F2, *b1 = F2 + 3, *b2 = F2 + 6, *d0 = D, *d1 = D + 3, *d2 = D + 6;
    c[0] = cons_det3(b0, b1, b2);
    c[1] = (cons_det3(d0, b1, b2) + cons_det3(b0, d1, b2)) + cons_det3(b0, b1, d2);
    c[2] = (cons_det3(b0, d1, d2) + cons_det3(d0, b1, d2)) + cons_det3(d0, d1, b2);
    c[3] = cons_det3(d0, d1, d2);
}
// T = [s 0 -s mx; 0 s -s my; 0 0 1] per view (N = mx1, my1, s1, mx2, my2, s2): F = T2^T Fn T1, scaled to unit Frobenius norm.
// false if the result is not finite or zero.
SRL_CONS_FN bool cons_denormalise(const double *Fn, const double *N, double *F) {
    double G[9];
    for (int i = 0; i < 3; i++) {
        G[3 * i] = Fn[3 * i] * N[2];
        G[3 * i + 1] = Fn[3 * i + 1] * N[2];
        G[3 * i + 2] = Fn[3 * i + 2] - N[2] * (N[0] * Fn[3 * i] + N[1] * Fn[3 * i + 1]);
    }
    double sq = 0.0;
    for (int j = 0; j < 3; j++) {
        F[j] = N[5] * G[j];
        F[3 + j] = N[5] * G[3 + j];
        F[6 + j] = G[6 + j] - N[5] * (N[3] * G[j] + N[4] * G[3 + j]);
    }
    for (int k = 0; k < 9; k++) sq += F[k] * F[k];
    const double norm = std::sqrt(sq);
    if (!(norm > 0.0) || !std::isfinite(norm)) return false;
    for (int k = 0; k < 9; k++) F[k] /= norm;
    double sq2 = 0.0;
    for (int k = 0; k < 9; k++) sq2 += F[k] * F[k];
    return std::isfinite(sq2) && sq2 > 0.5;
}

// ------------------------------------------------------------------------------------------------ P3P
// Grunert's solution as stated by Haralick, Lee, Ottenberg and Noelle (IJCV 13, 1994, eqs. 8-9): with the distances s1, s2 = u s1,
// s3 = v s1 of the three points from the centre, a quartic in v; every real root gives (s1, s2, s3), refined by three Newton steps on
//   s2^2 + s3^2 - 2 s2 s3 cos(alpha) = a^2,  s1^2 + s3^2 - 2 s1 s3 cos(beta) = b^2,  s1^2 + s2^2 - 2 s1 s2 cos(gamma) = c^2,
// and kept if all three are positive and the refined residual is at rounding level.  R, t then follow from the two congruent triangles
// (an orthonormal frame on each).  P: the three points (world), J: their unit bearings (camera).  out: 12 doubles per solution, written
// as they are accepted (the kernel hands in the hypothesis' model slots in global memory: no pose is staged in a per-lane array).
SRL_CONS_FN void cons_cross(const double *a, const double *b, double *c) {
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
SRL_CONS_FN double cons_dot(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
SRL_CONS_FN bool cons_frame(const double *p1, const double *p2, const double *p3, double *E) {      // E: rows e1, e2, e3
    double d12[3], d13[3];
    for (int k = 0; k < 3; k++) { d12[k] = p2[k] - p1[k]; d13[k] = p3[k] - p1[k]; }
    const double n1 = std::sqrt(cons_dot(d12, d12));
    for (int k = 0; k < 3; k++) E[k] = d12[k] / n1;
    cons_cross(E, d13, E + 6);
    const double n3 = std::sqrt(cons_dot(E + 6, E + 6));
    for (int k = 0; k < 3; k++) E[6 + k] /= n3;
    cons_cross(E + 6, E, E + 3);
    return n1 > 0.0 && n3 > 0.0;
}
SRL_CONS_FN int cons_p3p(const double *P, const double *J, double *out) {
    const double *P1 = P, *P2 = P + 3, *P3 = P + 6, *J1 = J, *J2 = J + 3, *J3 = J + 6;
    double d23[3], d13[3], d12[3], cr[3];
    for (int k = 0; k < 3; k++) { d23[k] = P2[k] - P3[k]; d13[k] = P1[k] - P3[k]; d12[k] = P1[k] - P2[k]; }
    const double a2 = cons_dot(d23, d23), b2 = cons_dot(d13, d13), c2 = cons_dot(d12, d12);
    cons_cross(d12, d13, cr);
    if (!(a2 > 0.0 && b2 > 0.0 && c2 > 0.0) || !(cons_dot(cr, cr) > 1e-12 * b2 * c2)) return 0;      // repeated or collinear points
    cons_cross(J2, J3, cr);
    if (!(std::fabs(cons_dot(J1, cr)) > 1e-12)) return 0;                                            // repeated or collinear image points
    const double ca = cons_dot(J2, J3), cb = cons_dot(J1, J3), cg = cons_dot(J1, J2);
    const double q1 = (a2 - c2) / b2, q2 = (a2 + c2) / b2, q3 = (b2 - c2) / b2, q4 = (b2 - a2) / b2, ra = a2 / b2, rc = c2 / b2;
    double A[5];
    A[4] = (q1 - 1.0) * (q1 - 1.0) - 4.0 * rc * ca * ca;
    A[3] = 4.0 * (q1 * (1.0 - q1) * cb - (1.0 - q2) * ca * cg + 2.0 * rc * ca * ca * cb);
    A[2] = 2.0 * (q1 * q1 - 1.0 + 2.0 * q1 * q1 * cb * cb + 2.0 * q3 * ca * ca - 4.0 * q2 * ca * cb * cg + 2.0 * q4 * cg * cg);
    A[1] = 4.0 * (-q1 * (1.0 + q1) * cb + 2.0 * ra * cg * cg * cb - (1.0 - q2) * ca * cg);
    A[0] = (1.0 + q1) * (1.0 + q1) - 4.0 * ra * cg * cg;
    double vr[4];
    cons_quartic(A, vr);
    int n = 0;
    for (int k = 0; k < 4; k++) {
        const double v = vr[k];
        if (!std::isfinite(v)) continue;
        const double den = 2.0 * (cg - v * ca), dd = (1.0 + v * v) - 2.0 * v * cb;
        if (!(std::fabs(den) > 1e-14) || !(dd > 0.0)) continue;
        const double u = ((q1 - 1.0) * v * v - 2.0 * q1 * cb * v + 1.0 + q1) / den;
        double s1 = std::sqrt(b2 / dd), s2 = u * s1, s3 = v * s1;
        double f1 = 0.0, f2 = 0.0, f3 = 0.0;
        for (int it = 0; it < 4; it++) {
            f1 = (s2 * s2 + s3 * s3 - 2.0 * s2 * s3 * ca) - a2;
            f2 = (s1 * s1 + s3 * s3 - 2.0 * s1 * s3 * cb) - b2;
            f3 = (s1 * s1 + s2 * s2 - 2.0 * s1 * s2 * cg) - c2;
            if (it == 3) break;
            // Jacobian rows: d f1 = (0, j12, j13), d f2 = (j21, 0, j23), d f3 = (j31, j32, 0)
            const double j12 = 2.0 * (s2 - s3 * ca), j13 = 2.0 * (s3 - s2 * ca), j21 = 2.0 * (s1 - s3 * cb), j23 = 2.0 * (s3 - s1 * cb),
                         j31 = 2.0 * (s1 - s2 * cg), j32 = 2.0 * (s2 - s1 * cg);
            const double det = j12 * j23 * j31 + j13 * j21 * j32;
            if (!(std::fabs(det) > 0.0)) break;
            // Cramer
            const double x1 = (-f1 * j23 * j32 + j12 * j23 * f3 + j13 * f2 * j32) / det;
            const double x2 = (f1 * j23 * j31 + j13 * j21 * f3 - j13 * f2 * j31) / det;
            const double x3 = (j12 * f2 * j31 + f1 * j21 * j32 - j12 * j21 * f3) / det;
            if (!(std::isfinite(x1) && std::isfinite(x2) && std::isfinite(x3))) break;
            s1 -= x1; s2 -= x2; s3 -= x3;
        }
        if (!(s1 > 0.0 && s2 > 0.0 && s3 > 0.0)) continue;
        if (!(std::fabs(f1) + std::fabs(f2) + std::fabs(f3) <= 1e-9 * ((a2 + b2) + c2))) continue;
        double Q[9], E[9], G[9];
        for (int i = 0; i < 3; i++) { Q[i] = s1 * J1[i]; Q[3 + i] = s2 * J2[i]; Q[6 + i] = s3 * J3[i]; }
        if (!cons_frame(P1, P2, P3, E) || !cons_frame(Q, Q + 3, Q + 6, G)) continue;
        double M[12];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) M[3 * i + j] = (G[i] * E[j] + G[3 + i] * E[3 + j]) + G[6 + i] * E[6 + j];
        for (int i = 0; i < 3; i++) M[9 + i] = Q[i] - ((M[3 * i] * P1[0] + M[3 * i + 1] * P1[1]) + M[3 * i + 2] * P1[2]);
        bool finite = true;
        for (int i = 0; i < 12; i++) finite = finite && std::isfinite(M[i]);
        if (!finite) continue;
        for (int i = 0; i < 12; i++) out[12 * n + i] = M[i];
        n++;
    }
    return n;
}
