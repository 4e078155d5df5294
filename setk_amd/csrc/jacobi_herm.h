// jacobi_herm.h -- the cyclic Jacobi eigendecomposition of a small Hermitian matrix in float64
// that the general CGMM EM (cgmm_k.hip) and the CACGMM EM (cacgmm.hip) share: numpy.linalg.eigh
// of Covariance (funcwj/setk scripts/sptk/libs/cluster.py:94-113) on the device.
#pragma once
#include <hip/hip_runtime.h>

namespace setk {

struct zc {
    double x, y;
};
__device__ __forceinline__ zc zmk(double a, double b) { return zc{a, b}; }

// cyclic Jacobi of the Hermitian A (n x n, row major, in place: diagonal = eigenvalues),
// V = eigenvectors in columns.  The rotation of (p, q) with a_pq = g e, |e| = 1:
//   U = [[c, s e], [-s conj(e), c]],  A <- U^H A U,  V <- V U
// (checked against numpy.linalg.eigh in the form of /tmp's numpy twin: eigenvalues 5e-15,
// residual 3e-15 at n = 16).
// Returns false when the sweep limit was reached with rotations still pending.
__device__ inline bool jacobi_herm(zc* A, zc* V, int n) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) V[i * n + j] = zmk(i == j ? 1.0 : 0.0, 0.0);
    // an off-diagonal entry below the rounding level of the matrix is left alone: a rotation
    // cannot make it smaller (its own arithmetic errs by ~eps trace), and a rank-deficient
    // covariance -- more channels than sources: a_pp a_qq ~ 0 -- would otherwise rotate through all
    // 60 sweeps at that level, in 220 of 257 bins of a 9-channel scene.  This is LAPACK's accuracy
    // class too (absolute in the norm of the matrix); eigenvalues down there are floored at
    // eps_float32 lambda_max afterwards (cluster.py:107-113)
    double tr = 0.0;
    for (int i = 0; i < n; ++i) tr += fabs(A[i * n + i].x);
    const double abs2 = 1.6e-31 * tr * tr;  // (4e-16 trace)^2
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rot = false;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const zc apq = A[p * n + q];
                const double g2 = apq.x * apq.x + apq.y * apq.y;
                const double app = A[p * n + p].x, aqq = A[q * n + q].x;
                if (!(g2 > 1e-34 * fabs(app * aqq)) || !(g2 > abs2) || g2 == 0.0) continue;
                rot = true;
                const double g = sqrt(g2);
                const double ex = apq.x / g, ey = apq.y / g;
                const double tau = (aqq - app) / (2.0 * g);
                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
                const double sx = s * ex, sy = s * ey;  // s e
                for (int i = 0; i < n; ++i) {  // columns p, q of A and of V
                    for (int m = 0; m < 2; ++m) {
                        zc* M = m ? V : A;
                        const zc cp = M[i * n + p], cq = M[i * n + q];
                        // new p = c cp - s conj(e) cq ; new q = s e cp + c cq
                        M[i * n + p] = zmk(c * cp.x - (sx * cq.x + sy * cq.y), c * cp.y - (sx * cq.y - sy * cq.x));
                        M[i * n + q] = zmk((sx * cp.x - sy * cp.y) + c * cq.x, (sx * cp.y + sy * cp.x) + c * cq.y);
                    }
                }
                for (int j = 0; j < n; ++j) {  // rows p, q of A
                    const zc rp = A[p * n + j], rq = A[q * n + j];
                    // new p = c rp - s e rq ; new q = s conj(e) rp + c rq
                    A[p * n + j] = zmk(c * rp.x - (sx * rq.x - sy * rq.y), c * rp.y - (sx * rq.y + sy * rq.x));
                    A[q * n + j] = zmk((sx * rp.x + sy * rp.y) + c * rq.x, (sx * rp.y - sy * rp.x) + c * rq.y);
                }
            }
        if (!rot) return true;
    }
    return false;
}

}  // namespace setk
