// Eigen-decomposition of a symmetric 4 x 4 matrix in fp64 by cyclic Jacobi rotations: sym_eig3.h's rotation (Rutishauser's form, a
// pair whose a_pq is zero already is left alone bit for bit) in the fixed pair order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) and a FIXED
// number of sweeps: no convergence test, no loop whose length depends on the data.  Every index is a compile-time constant once the
// loops are unrolled, so the two arrays live in registers and nothing goes to scratch.  tests/corr_ransac_ref.py restates it.
#pragma once

#ifndef PN2_HORN_SWEEPS
#define PN2_HORN_SWEEPS 8
#endif

template <int P, int Q>
__host__ __device__ __forceinline__ void pn2_jacobi4_rotate(double (&A)[4][4], double (&V)[4][4]) {
    const double apq = A[P][Q];
    const bool on = apq != 0.0;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);           // (off: inf or NaN, discarded below)
    double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));       // the smaller root; theta^2 = inf gives t = 0
    t = theta < 0.0 ? -t : t;
    t = on ? t : 0.0;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    const double h = t * (on ? apq : 0.0);
    A[P][P] = on ? A[P][P] - h : A[P][P];
    A[Q][Q] = on ? A[Q][Q] + h : A[Q][Q];
    A[P][Q] = A[Q][P] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r == P || r == Q) continue;
        const double rp = A[r][P], rq = A[r][Q];
        A[r][P] = A[P][r] = on ? c * rp - s * rq : rp;
        A[r][Q] = A[Q][r] = on ? s * rp + c * rq : rq;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double vp = V[k][P], vq = V[k][Q];
        V[k][P] = on ? c * vp - s * vq : vp;
        V[k][Q] = on ? s * vp + c * vq : vq;
    }
}

// A (symmetric, overwritten: its diagonal ends as the eigenvalues, unsorted) -> u = the eigenvector of the LARGEST diagonal entry,
// the first among equals (strict >), as a column of the accumulated rotations; returns that eigenvalue.
__host__ __device__ __forceinline__ double pn2_sym_eig4_largest(double (&A)[4][4], double (&u)[4]) {
    double V[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) V[r][c] = r == c ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < PN2_HORN_SWEEPS; ++sweep) {
        pn2_jacobi4_rotate<0, 1>(A, V);
        pn2_jacobi4_rotate<0, 2>(A, V);
        pn2_jacobi4_rotate<0, 3>(A, V);
        pn2_jacobi4_rotate<1, 2>(A, V);
        pn2_jacobi4_rotate<1, 3>(A, V);
        pn2_jacobi4_rotate<2, 3>(A, V);
    }
    double best = A[0][0];
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k] = V[k][0];
#pragma unroll
    for (int c = 1; c < 4; ++c) {
        const bool take = A[c][c] > best;
        best = take ? A[c][c] : best;
#pragma unroll
        for (int k = 0; k < 4; ++k) u[k] = take ? V[k][c] : u[k];
    }
    return best;
}
