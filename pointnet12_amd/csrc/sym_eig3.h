// Eigen-decomposition of a symmetric 3 x 3 matrix in fp64 by cyclic Jacobi rotations with a FIXED number of sweeps: no
// convergence test, no loop whose length depends on the data, no array (nine + six scalars, nothing goes to scratch).
//
// One rotation annihilates a_pq exactly (Rutishauser's form: the diagonal moves by t a_pq, which keeps small eigenvalues of a
// graded matrix accurate); a pair whose a_pq is already zero is left alone bit for bit (t = 0 -> c = 1, s = 0), so a diagonal
// matrix comes back as it went in with V = I -- the axis-aligned planes and lines give their axis exactly.  Cyclic Jacobi converges
// quadratically: on 3 x 3 matrices the off-diagonal norm is below 2^-53 of the largest eigenvalue after four sweeps (6e-21 of it on
// 700 000 matrices of condition 1 .. 1e30 and with eigenvalues 1e-13 apart; tests/test_normals_cpu.py restates the iteration and
// counts), PN2_PCA_SWEEPS = 6 leaves two in hand.  A sweep over a matrix that is diagonal already changes nothing.
#pragma once

#ifndef PN2_PCA_SWEEPS
#define PN2_PCA_SWEEPS 6
#endif

// rotation in the (p, q) plane; r is the third index.  v?p / v?q: the two affected columns of V.
__host__ __device__ __forceinline__ void pn2_jacobi_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p,
                                                            double &v0q, double &v1p, double &v1q, double &v2p, double &v2q) {
    const bool on = apq != 0.0;
    const double theta = (aqq - app) / (2.0 * apq);                   // (off: inf or NaN, discarded below)
    double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));       // the smaller root; theta^2 = inf gives t = 0
    t = theta < 0.0 ? -t : t;
    t = on ? t : 0.0;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    const double h = t * apq;
    app = on ? app - h : app;
    aqq = on ? aqq + h : aqq;
    apq = 0.0;
    const double rp = arp, rq = arq;
    arp = on ? c * rp - s * rq : rp;
    arq = on ? s * rp + c * rq : rq;
    const double a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
    v0p = on ? c * a0 - s * b0 : a0;
    v0q = on ? s * a0 + c * b0 : b0;
    v1p = on ? c * a1 - s * b1 : a1;
    v1q = on ? s * a1 + c * b1 : b1;
    v2p = on ? c * a2 - s * b2 : a2;
    v2q = on ? s * a2 + c * b2 : b2;
}

// C = (xx, xy, xz, yy, yz, zz) -> l[0] <= l[1] <= l[2] (as computed: the caller clamps) and u = the eigenvector of l[0].
// Equal diagonal entries keep their axis order (the lowest axis is l[0]'s).
__host__ __device__ __forceinline__ void pn2_sym_eig3(double xx, double xy, double xz, double yy, double yz, double zz, double &l0, double &l1,
                                                       double &l2, double &ux, double &uy, double &uz) {
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    for (int sweep = 0; sweep < PN2_PCA_SWEEPS; ++sweep) {
        pn2_jacobi_rotate(xx, yy, xy, xz, yz, v00, v01, v10, v11, v20, v21);      // (0, 1), r = 2
        pn2_jacobi_rotate(xx, zz, xz, xy, yz, v00, v02, v10, v12, v20, v22);      // (0, 2), r = 1
        pn2_jacobi_rotate(yy, zz, yz, xy, xz, v01, v02, v11, v12, v21, v22);      // (1, 2), r = 0
    }
    // the smallest diagonal entry, the first among equals (strict <)
    const bool y_lt_x = yy < xx;
    const double m01 = y_lt_x ? yy : xx;
    const bool z_lt = zz < m01;
    l0 = z_lt ? zz : m01;
    ux = z_lt ? v02 : (y_lt_x ? v01 : v00);
    uy = z_lt ? v12 : (y_lt_x ? v11 : v10);
    uz = z_lt ? v22 : (y_lt_x ? v21 : v20);
    const double hi01 = y_lt_x ? xx : yy;                                        // the larger of xx, yy
    const double big = zz > hi01 ? zz : hi01;
    l2 = big;
    l1 = z_lt ? m01 : (zz > hi01 ? hi01 : zz);
}
