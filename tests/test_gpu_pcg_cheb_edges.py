"""cfs_hip_sym_pcg_cheb, cfs_hip_sym_cheb_apply and cfs_hip_sym_precond_lmax where test_gpu_pcg_cheb_steps.py stops,
by its method and with its CPU side (Problem, poly_reference, pcg_cheb_reference, power_reference): the long-double
recurrence is the reference, d the deviation of the same recurrence in the working precision with the kernels'
rounding rules, the GPU is allowed 4 d + 16 u, a case with d > D_LIMIT is badly chosen and fails.  Bounds are passed
explicitly: lmax = the Gershgorin bound of M^-1 A, lmin = lmax / 30.

1. Every block size.  The kernels of csrc/cfs_solver_cheb.hpp are instantiated for BS = 0, 1, 2, 3, 4, 6 and the steps
file runs 0, 1, 3.  Here bs = 2, 4, 6 on rand65, rand1026 (neither n divisible by 4 or 6: a partial last block) and
rotated_node_blocks(bs): the polynomial (m = 1, 2, 5), the iterates (k = 1, 2, 3, 5, 10; m = 1, 3), the power
method (16 steps, explicit and default v0).  bs = 1 through the block entry is the Jacobi base, bit for bit.

2. Beyond one trip of the grid (512 x 256 threads): band600001, n mod 2, 3, 4 = 1.  The vector loops of the
diagonal forms take a second trip for n > 262 144 (fp64) / 524 288 (fp32), the scalar loops of the power method for
n > 131 072, the block forms for more than 131 072 node blocks (300 001, 200 001, 150 001 for bs = 2, 3, 4).
cheb_apply at m = 3, iterates k = 1, 2 at m = 2 (and m = 1 with Jacobi: cheb_update_kernel's with_rz path), the
power method with 4 steps.  For bs = 6 a band matrix of 800 003 rows (133 334 blocks, the last of 5 rows), fp64,
cheb_apply at m = 2.

3. High degree: m = 8 and 16 (the coefficient arrays hold 16 entries; the cap on the window of enqueued iterations,
80 / (5 + 3 (m - 1)), is 4 at m = 6 and 1 at m = 16) on rand1023 and pwtk@0.05; iterates k = 1, 2, 3 at m = 6, 16;
on a deterministic handle a converging solve gives the same bytes and count for check_every = 1, 3, 1000.

4. A first guess that is not zero: k = 1, 2, 5 from x0 uniform in (-1, 1), m = 3 -- q = A x0 feeds the first residual.

Measured on the MI355X (d / the GPU's deviation):

  every block size, z = P_m r for m = 1, 2, 5; then 16 power steps from the explicit / the default v0:
    f64 rand65    bs=2  1.5e-16/1.5e-16  1.2e-16/7.4e-17  7.7e-17/9.2e-17    2.0e-16/8.9e-17  4.8e-17/4.8e-17
    f32 rand65    bs=2  3.3e-08/3.3e-08  4.5e-08/4.5e-08  5.4e-08/5.4e-08    2.0e-08/2.0e-08  6.7e-09/6.1e-09
    f64 rand1026  bs=2  1.1e-16/1.1e-16  1.2e-16/6.8e-17  1.1e-16/1.8e-16    4.2e-17/4.2e-17  3.0e-17/3.0e-17
    f32 rand1026  bs=2  1.9e-08/1.9e-08  5.2e-08/5.2e-08  6.0e-08/6.0e-08    1.2e-09/4.3e-09  1.0e-08/4.2e-09
    f64 rotated2  bs=2  2.1e-16/1.9e-16  6.5e-16/6.2e-16  2.2e-15/2.7e-15    5.4e-17/2.7e-16  2.2e-16/2.7e-16
    f32 rotated2  bs=2  4.8e-08/4.8e-08  3.1e-07/1.8e-07  1.3e-06/7.3e-07    1.8e-09/6.4e-10  4.8e-10/2.0e-09
    f64 rand65    bs=4  2.3e-16/9.4e-17  1.7e-16/1.1e-16  1.7e-16/5.3e-17    5.0e-17/9.7e-17  8.0e-17/6.4e-17
    f32 rand65    bs=4  3.3e-08/3.3e-08  3.4e-08/3.4e-08  4.5e-08/4.5e-08    1.0e-08/4.5e-09  1.8e-08/8.4e-09
    f64 rand1026  bs=4  1.1e-16/1.1e-16  1.2e-16/8.4e-17  1.4e-16/1.1e-16    2.7e-16/1.5e-17  8.4e-17/6.0e-17
    f32 rand1026  bs=4  1.9e-08/1.9e-08  5.2e-08/5.2e-08  6.0e-08/6.0e-08    1.4e-09/8.0e-09  9.9e-09/3.3e-10
    f64 rotated4  bs=4  2.3e-16/2.0e-16  4.1e-15/4.5e-15  1.7e-14/1.6e-14    3.2e-16/4.3e-18  4.0e-19/1.6e-16
    f32 rotated4  bs=4  4.5e-08/4.5e-08  2.5e-06/1.3e-06  1.3e-05/5.9e-06    8.3e-09/5.0e-09  3.3e-08/2.0e-08
    f64 rand65    bs=6  2.2e-16/9.9e-17  1.8e-16/8.7e-17  1.4e-16/3.9e-17    1.6e-17/1.6e-17  6.9e-17/7.8e-17
    f32 rand65    bs=6  2.0e-08/2.0e-08  3.8e-08/3.8e-08  9.2e-08/9.2e-08    2.2e-10/3.8e-09  7.9e-09/1.1e-08
    f64 rand1026  bs=6  1.1e-16/1.1e-16  1.2e-16/8.4e-17  1.1e-16/1.1e-16    3.1e-17/1.8e-16  1.9e-16/2.5e-16
    f32 rand1026  bs=6  1.9e-08/1.9e-08  5.2e-08/5.2e-08  6.0e-08/6.0e-08    4.2e-09/8.3e-09  5.2e-09/2.9e-10
    f64 rotated6  bs=6  2.2e-16/1.6e-16  5.8e-15/7.4e-15  2.0e-14/1.8e-14    1.2e-15/3.0e-16  3.0e-16/3.0e-16
    f32 rotated6  bs=6  3.9e-08/3.9e-08  2.7e-06/1.5e-06  1.5e-05/7.0e-06    3.0e-07/4.4e-07  2.4e-07/5.9e-08

  every block size, iterates k = 1, 2, 3, 5, 10:
    f64 rand65    bs=2 m=1  1.2e-16/1.5e-16  1.7e-16/2.4e-16  1.7e-16/2.6e-16  2.2e-16/3.7e-16  2.6e-16/4.4e-16
    f64 rand65    bs=2 m=3  1.8e-16/7.1e-17  1.4e-16/1.2e-16  2.2e-16/2.2e-16  2.4e-16/2.4e-16  4.1e-16/4.1e-16
    f32 rand65    bs=2 m=1  6.4e-08/6.4e-08  1.0e-07/1.0e-07  1.2e-07/1.2e-07  1.8e-07/1.8e-07  1.9e-07/1.9e-07
    f32 rand65    bs=2 m=3  6.5e-08/1.1e-07  6.3e-08/8.1e-08  5.6e-08/1.2e-07  4.2e-08/1.0e-07  7.8e-08/1.2e-07
    f64 rand1026  bs=2 m=1  1.1e-16/2.0e-16  9.7e-17/9.5e-17  1.3e-16/1.0e-16  1.5e-16/1.0e-16  1.6e-16/2.1e-16
    f64 rand1026  bs=2 m=3  9.0e-17/2.2e-16  1.2e-16/1.1e-16  2.2e-16/1.3e-16  2.9e-16/1.4e-16  4.5e-16/2.3e-16
    f32 rand1026  bs=2 m=1  3.6e-08/3.6e-08  4.1e-08/3.4e-08  4.6e-08/4.6e-08  7.5e-08/7.5e-08  9.4e-08/9.4e-08
    f32 rand1026  bs=2 m=3  4.6e-08/4.6e-08  5.1e-08/5.1e-08  5.9e-08/5.9e-08  6.8e-08/6.8e-08  1.5e-07/1.5e-07
    f64 rotated2  bs=2 m=1  3.2e-16/3.5e-16  1.6e-15/1.6e-15  1.6e-15/1.6e-15  1.6e-15/1.6e-15  1.6e-15/1.6e-15
    f64 rotated2  bs=2 m=3  1.4e-15/1.4e-15  1.7e-15/2.0e-15  1.7e-15/1.9e-15  1.7e-15/1.8e-15  1.8e-15/1.9e-15
    f32 rotated2  bs=2 m=1  9.1e-08/9.0e-08  7.6e-07/4.2e-07  7.9e-07/4.2e-07  8.0e-07/4.0e-07  8.5e-07/4.6e-07
    f32 rotated2  bs=2 m=3  7.1e-07/4.2e-07  1.0e-06/5.1e-07  1.0e-06/5.2e-07  1.0e-06/5.7e-07  9.9e-07/5.8e-07
    f64 rand65    bs=4 m=1  4.1e-16/1.8e-16  2.9e-16/1.4e-16  2.6e-16/7.8e-17  1.6e-16/7.1e-17  2.5e-16/8.8e-17
    f64 rand65    bs=4 m=3  2.0e-16/2.0e-16  1.6e-16/1.6e-16  1.4e-16/1.3e-16  1.5e-16/1.5e-16  2.5e-16/2.5e-16
    f32 rand65    bs=4 m=1  5.6e-08/5.6e-08  9.6e-08/7.0e-08  1.3e-07/8.6e-08  1.1e-07/4.5e-08  8.0e-08/8.0e-08
    f32 rand65    bs=4 m=3  6.0e-08/6.0e-08  1.1e-07/1.1e-07  7.4e-08/7.4e-08  6.6e-08/1.0e-07  1.6e-07/1.6e-07
    f64 rand1026  bs=4 m=1  6.9e-17/6.9e-17  8.6e-17/7.3e-17  1.2e-16/9.6e-17  9.7e-17/1.2e-16  1.4e-16/1.4e-16
    f64 rand1026  bs=4 m=3  1.5e-16/1.6e-16  1.3e-16/9.7e-17  2.0e-16/1.4e-16  2.3e-16/1.6e-16  2.8e-16/1.8e-16
    f32 rand1026  bs=4 m=1  3.9e-08/3.9e-08  4.9e-08/4.9e-08  5.8e-08/5.2e-08  6.4e-08/7.4e-08  8.1e-08/1.0e-07
    f32 rand1026  bs=4 m=3  4.3e-08/4.3e-08  6.4e-08/6.4e-08  7.9e-08/7.9e-08  1.2e-07/1.2e-07  1.3e-07/1.3e-07
    f64 rotated4  bs=4 m=1  1.1e-15/1.0e-15  1.1e-13/1.2e-13  1.1e-13/1.1e-13  1.0e-13/1.1e-13  1.0e-13/1.1e-13
    f64 rotated4  bs=4 m=3  7.8e-15/6.9e-15  1.1e-13/1.1e-13  1.1e-13/1.1e-13  1.1e-13/1.1e-13  1.1e-13/1.1e-13
    f32 rotated4  bs=4 m=1  3.7e-07/1.2e-07  6.4e-05/3.3e-05  6.3e-05/3.3e-05  6.2e-05/3.2e-05  6.2e-05/3.2e-05
    f32 rotated4  bs=4 m=3  4.4e-06/2.6e-06  8.8e-05/3.0e-05  8.9e-05/3.4e-05  8.8e-05/3.4e-05  8.8e-05/3.4e-05
    f64 rand65    bs=6 m=1  2.2e-16/2.2e-16  1.1e-16/2.5e-16  1.3e-16/2.4e-16  1.4e-16/2.2e-16  3.8e-16/5.6e-16
    f64 rand65    bs=6 m=3  9.2e-17/2.4e-16  6.6e-17/1.9e-16  9.6e-17/2.0e-16  1.1e-16/7.2e-17  2.2e-16/2.2e-16
    f32 rand65    bs=6 m=1  2.4e-08/4.7e-08  5.7e-08/3.8e-08  1.1e-07/7.9e-08  1.5e-07/1.5e-07  1.7e-07/1.8e-07
    f32 rand65    bs=6 m=3  7.1e-08/7.1e-08  9.9e-08/9.9e-08  9.4e-08/9.4e-08  9.9e-08/9.9e-08  8.4e-08/8.4e-08
    f64 rand1026  bs=6 m=1  1.0e-16/1.7e-16  7.4e-17/7.1e-17  8.5e-17/1.2e-16  1.4e-16/1.2e-16  1.7e-16/1.4e-16
    f64 rand1026  bs=6 m=3  3.2e-16/9.8e-17  1.0e-16/1.2e-16  1.2e-16/1.4e-16  1.8e-16/1.5e-16  3.2e-16/2.3e-16
    f32 rand1026  bs=6 m=1  3.3e-08/3.3e-08  5.8e-08/6.4e-08  7.0e-08/1.1e-07  8.3e-08/1.7e-07  1.3e-07/2.1e-07
    f32 rand1026  bs=6 m=3  6.0e-08/6.0e-08  1.0e-07/1.0e-07  9.7e-08/9.7e-08  8.0e-08/6.0e-08  8.4e-08/9.3e-08
    f64 rotated6  bs=6 m=1  4.2e-15/2.3e-16  2.7e-13/3.5e-13  2.8e-13/3.6e-13  2.8e-13/3.6e-13  2.8e-13/3.6e-13
    f64 rotated6  bs=6 m=3  1.3e-14/1.1e-14  3.3e-13/2.6e-13  3.3e-13/2.8e-13  3.3e-13/2.7e-13  3.3e-13/2.7e-13
    f32 rotated6  bs=6 m=1  2.5e-06/1.3e-07  1.3e-04/7.0e-05  1.3e-04/7.3e-05  1.3e-04/7.2e-05  1.3e-04/7.2e-05
    f32 rotated6  bs=6 m=3  6.4e-06/3.6e-06  1.3e-04/7.5e-05  1.4e-04/7.7e-05  1.4e-04/7.6e-05  1.4e-04/7.6e-05

  band600001 (band800003 for bs = 6), z = P_m r:
    f64 band600001 none              m=3 2.9e-16/2.6e-16
    f32 band600001 none              m=3 1.2e-07/1.2e-07
    f64 band600001 jacobi            m=3 3.0e-16/2.7e-16
    f32 band600001 jacobi            m=3 1.3e-07/1.3e-07
    f64 band600001 block_jacobi bs=2 m=3 2.4e-16/2.5e-16
    f64 band600001 block_jacobi bs=3 m=3 2.6e-16/2.3e-16
    f64 band600001 block_jacobi bs=4 m=3 2.3e-16/2.3e-16
    f64 band800003 block_jacobi bs=6 m=2 2.8e-16/3.2e-16

  band600001, iterates k = 1, 2:
    f64 none              m=2  2.8e-16/2.7e-16  4.8e-16/3.5e-16
    f32 none              m=2  1.6e-07/1.2e-07  1.5e-07/1.3e-07
    f64 jacobi            m=2  5.6e-16/3.1e-16  4.2e-16/4.4e-16
    f64 jacobi            m=1  3.0e-16/3.0e-16  3.4e-16/3.8e-16
    f32 jacobi            m=2  1.3e-07/1.3e-07  2.0e-07/1.6e-07
    f32 jacobi            m=1  1.2e-07/1.2e-07  1.6e-07/1.3e-07
    f64 block_jacobi bs=2 m=2  3.2e-16/2.7e-16  3.4e-16/3.9e-16
    f64 block_jacobi bs=3 m=2  4.4e-16/3.2e-16  3.7e-16/4.0e-16
    f64 block_jacobi bs=4 m=2  3.8e-16/2.7e-16  3.7e-16/4.3e-16

  band600001, 4 power steps from the explicit / the default v0:
    f64 jacobi            1.7e-16/3.0e-16  1.2e-16/4.4e-16
    f32 jacobi            2.4e-10/6.7e-11  6.3e-11/6.6e-11
    f64 block_jacobi bs=2 2.7e-16/8.7e-16  2.9e-16/7.7e-16
    f64 block_jacobi bs=3 5.1e-17/7.2e-16  3.2e-16/1.0e-15
    f64 block_jacobi bs=4 8.9e-17/6.1e-16  1.3e-16/9.1e-16

  high degree, z = P_m r for m = 8, 16:
    f64 rand1023  none          2.0e-16/2.3e-16  3.3e-16/3.3e-16
    f64 rand1023  jacobi        2.0e-16/2.0e-16  1.8e-16/1.8e-16
    f64 rand1023  block_jacobi  1.7e-16/1.7e-16  1.6e-16/1.7e-16
    f32 rand1023  none          1.3e-07/1.3e-07  1.6e-07/1.6e-07
    f32 rand1023  jacobi        4.4e-08/4.4e-08  7.2e-08/7.2e-08
    f32 rand1023  block_jacobi  4.4e-08/4.4e-08  5.3e-08/5.3e-08
    f64 pwtk@0.05 none          3.0e-16/3.0e-16  3.0e-16/3.8e-16
    f64 pwtk@0.05 jacobi        1.1e-16/1.4e-16  1.5e-16/1.8e-16
    f32 pwtk@0.05 none          1.5e-07/1.5e-07  1.8e-07/1.8e-07
    f32 pwtk@0.05 jacobi        5.9e-08/5.9e-08  6.7e-08/9.1e-08

  high degree, iterates k = 1, 2, 3:
    f64 rand1023  none         m=6   2.9e-16/2.2e-16  7.1e-16/3.2e-16  1.2e-15/3.2e-16
    f64 rand1023  none         m=16  3.5e-16/3.7e-16  3.5e-16/3.7e-16  3.2e-16/3.2e-16
    f64 rand1023  jacobi       m=6   3.8e-16/8.9e-17  1.4e-16/1.2e-16  1.9e-16/1.9e-16
    f64 rand1023  jacobi       m=16  2.1e-16/2.9e-16  1.4e-16/2.1e-16  1.5e-16/1.3e-16
    f64 rand1023  block_jacobi m=6   1.8e-16/3.7e-16  1.7e-16/1.3e-16  1.9e-16/1.9e-16
    f64 rand1023  block_jacobi m=16  2.7e-16/2.7e-16  2.1e-16/1.1e-16  1.8e-16/1.4e-16
    f32 rand1023  none         m=6   1.3e-07/1.3e-07  9.8e-08/1.0e-07  1.0e-07/1.5e-07
    f32 rand1023  none         m=16  1.9e-07/1.9e-07  1.4e-07/1.4e-07  1.6e-07/1.6e-07
    f32 rand1023  jacobi       m=6   4.9e-08/4.9e-08  8.2e-08/8.2e-08  9.2e-08/9.2e-08
    f32 rand1023  jacobi       m=16  8.5e-08/8.5e-08  6.6e-08/7.6e-08  9.7e-08/9.7e-08
    f32 rand1023  block_jacobi m=6   4.2e-08/4.2e-08  6.6e-08/6.6e-08  8.3e-08/8.6e-08
    f32 rand1023  block_jacobi m=16  5.3e-08/5.3e-08  1.5e-07/1.5e-07  1.1e-07/1.1e-07
    f64 pwtk@0.05 none         m=6   3.0e-16/2.8e-16  4.2e-16/3.2e-16  4.5e-16/4.2e-16
    f64 pwtk@0.05 none         m=16  3.9e-16/4.5e-16  4.6e-16/3.7e-16  3.5e-16/4.2e-16
    f64 pwtk@0.05 jacobi       m=6   2.0e-16/1.7e-16  4.3e-16/3.4e-16  3.4e-16/2.4e-16
    f64 pwtk@0.05 jacobi       m=16  2.6e-16/1.6e-16  5.9e-16/3.5e-16  2.8e-16/2.0e-16
    f32 pwtk@0.05 none         m=6   1.6e-07/1.6e-07  2.4e-07/1.7e-07  2.0e-07/1.7e-07
    f32 pwtk@0.05 none         m=16  2.1e-07/2.1e-07  2.0e-07/1.9e-07  1.7e-07/1.7e-07
    f32 pwtk@0.05 jacobi       m=6   7.6e-08/7.6e-08  3.8e-07/1.4e-07  2.3e-07/8.7e-08
    f32 pwtk@0.05 jacobi       m=16  7.2e-08/8.2e-08  2.9e-07/1.6e-07  1.5e-07/9.9e-08

  converging solves on the deterministic handle (the same for check_every = 1, 3, 1000):
    f64 pwtk@0.05 jacobi m=6: 51 iterations, relres 8.722e-09
    f64 pwtk@0.05 jacobi m=16: 44 iterations, relres 7.040e-09
    f32 pwtk@0.05 jacobi m=6: 30 iterations, relres 8.961e-05
    f32 pwtk@0.05 jacobi m=16: 26 iterations, relres 7.171e-05

  from x0, m = 3, iterates k = 1, 2, 5:
    f64 rand257   none          6.4e-16/6.0e-16  1.5e-15/6.1e-16  4.9e-16/6.8e-16
    f64 rand257   jacobi        1.8e-16/1.8e-16  4.8e-16/1.6e-16  7.8e-16/2.4e-16
    f64 rand257   block_jacobi  1.4e-16/1.9e-16  2.6e-16/3.9e-16  2.1e-16/2.8e-16
    f32 rand257   none          3.0e-07/4.9e-07  3.3e-07/2.8e-07  3.7e-07/2.0e-07
    f32 rand257   jacobi        9.6e-08/9.6e-08  1.0e-07/7.2e-08  2.3e-07/9.0e-08
    f32 rand257   block_jacobi  1.4e-07/1.4e-07  8.1e-08/8.1e-08  1.4e-07/1.4e-07
    f64 pwtk@0.05 none          2.2e-15/1.7e-15  2.4e-15/1.4e-15  1.8e-15/7.1e-16
    f64 pwtk@0.05 jacobi        2.6e-16/2.1e-16  5.4e-16/3.8e-16  1.5e-15/8.9e-16
    f32 pwtk@0.05 none          1.3e-06/4.8e-07  1.2e-06/4.6e-07  7.3e-07/3.4e-07
    f32 pwtk@0.05 jacobi        1.4e-07/8.5e-08  3.1e-07/2.0e-07  7.5e-07/4.0e-07
"""
import numpy as np
import pytest

from test_gpu_cg_steps import DET, DTYPES
from test_gpu_lanczos_steps import default_v0
from test_gpu_pcg_cheb_steps import LD, Problem, _apply_gpu, _check_iterates, _native, _problem, poly_reference, power_reference
from test_gpu_kernel_variants import PLAN_KNOBS
from test_gpu_pcg_steps import D_LIMIT, KS, UNIT, _deviation, _matrix, _rhs, scaled

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _torch_first(monkeypatch):
    """torch brings a HIP runtime of its own: it has to initialise before libcfs_hip.so's"""
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    for k in PLAN_KNOBS + ("CFS_HIP_CG_GRAPH",):
        monkeypatch.delenv(k, raising=False)
    yield


def _f(dtype):
    return "f64" if dtype == np.float64 else "f32"


def _lmax_gpu(A, base, block, steps, v0):
    import torch
    return A.precond_lmax(base=base, block=block, steps=steps, v0=None if v0 is None else torch.from_numpy(v0).cuda())


def _check_apply(name, P, A, dtype, block, degrees, bounds=None):
    """z = P_m r on the GPU against the long-double recurrence, for every m of degrees"""
    lmin, lmax = bounds or P.bounds()
    x, errors = _rhs(P.n, dtype), []
    for m in degrees:
        ref = poly_reference(P, x, m, lmin, lmax)
        d = _deviation(poly_reference(P, x, m, lmin, lmax, dtype), ref)
        assert d <= D_LIMIT[dtype], f"{name} {P.base} m={m}: d = {d:.3e}: badly conditioned case"
        px = _apply_gpu(A, x, P.base, m, lmin, lmax, block=block)
        assert px.dtype == dtype
        g, allowed = _deviation(px, ref), 4 * d + 16 * UNIT[dtype]
        print(f"cheb-edges apply    {_f(dtype)} {name} {P.base} bs={block} n={P.n} m={m} bounds=({lmin:.4g}, {lmax:.4g}) "
              f"d={d:.3e} gpu={g:.3e} allowed={allowed:.3e}")
        if not (np.all(np.isfinite(px)) and g <= allowed):
            errors.append(f"{P.base} bs={block} m={m}: deviation {g:.3e}, allowed {allowed:.3e} (d = {d:.3e})")
    return errors


def _check_lmax(name, P, A, dtype, block, steps):
    """`steps` power steps from an explicit v0 and from the default one against the long-double power method"""
    errors = []
    for label, v0 in (("explicit v0", _rhs(P.n, dtype)), ("default v0", None)):
        start = default_v0(P.n).astype(dtype) if v0 is None else v0
        ref = power_reference(P, start, steps)
        d = float(abs(LD(power_reference(P, start, steps, dtype)) - ref) / abs(ref))
        assert d <= D_LIMIT[dtype], f"{name} {P.base}: d = {d:.3e}: badly conditioned case"
        est = _lmax_gpu(A, P.base, block, steps, v0)
        g, allowed = float(abs(LD(est) - ref) / abs(ref)), 4 * d + 16 * UNIT[dtype]
        print(f"cheb-edges estimate {_f(dtype)} {name} {P.base} bs={block} n={P.n} steps={steps} {label} est={est:.17g} "
              f"long double={float(ref):.17g} d={d:.3e} gpu={g:.3e} allowed={allowed:.3e}")
        if not g <= allowed:
            errors.append(f"{P.base} bs={block} {label}: estimate {est!r} against {float(ref)!r}: {g:.3e}, allowed {allowed:.3e}")
    return errors


def _iterates(name, P, A, b, dtype, block, m, ks, bounds=None, x0=None, label=""):
    lmin, lmax = bounds or P.bounds()
    return _check_iterates(name, P, b, dtype, m, lmin, lmax,
                           lambda k: _native(A, b, x0=x0, base=P.base, block=block, degree=m, lmin=lmin, lmax=lmax, tol=0.0,
                                             maxiter=k)[:2], label=f"{label} bs={block}", ks=ks, x0=x0)


# ---- 1. every block size ------------------------------------------------------------------------------------
BLOCK_CASES = [(name, bs) for bs in (2, 4, 6) for name in ("rand65", "rand1026", f"rotated{bs}")]
BLOCK_IDS = [f"{name}-bs{bs}" for name, bs in BLOCK_CASES]


@DTYPES
@pytest.mark.parametrize("name,bs", BLOCK_CASES, ids=BLOCK_IDS)
def test_every_block_size_polynomial_and_estimate(name, bs, dtype):
    P, A = _problem(name, dtype, "block_jacobi", block=bs)
    assert P.minv.shape == (-(-P.n // bs), bs, bs)
    errors = _check_apply(name, P, A, dtype, bs, (1, 2, 5)) + _check_lmax(name, P, A, dtype, bs, 16)
    A.close()
    assert not errors, f"{name} {_f(dtype)}: " + "; ".join(errors)


@DTYPES
@pytest.mark.parametrize("name,bs", BLOCK_CASES, ids=BLOCK_IDS)
def test_every_block_size_iterates(name, bs, dtype):
    P, A = _problem(name, dtype, "block_jacobi", block=bs)
    b = _rhs(P.n, dtype)
    errors = []
    for m in (1, 3):
        errors += _iterates(name, P, A, b, dtype, bs, m, KS)
    A.close()
    assert not errors, f"{name} {_f(dtype)}: " + "; ".join(errors)


@DTYPES
def test_block_one_through_the_block_entry_is_jacobi(dtype):
    """base = "block_jacobi" with block = 1 against base = "jacobi" on a deterministic handle: the same bits in u, the
    same count and reported residual; the same polynomial and the same estimate"""
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("rand1026")
    va, b = scaled(n, rp, ci, va, dtype), _rhs(n, dtype)
    D = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
    assert D.kernel_variant()["det"] == 1
    lmin, lmax = Problem(n, rp, ci, va, "jacobi").bounds()
    for kw in (dict(degree=1, tol=0.0, maxiter=7), dict(degree=3, tol=0.0, maxiter=7),
               dict(degree=3, tol=1e-8 if dtype == np.float64 else 1e-4, maxiter=500, check_every=3)):
        u1, it1, res1, used1 = _native(D, b, base="jacobi", lmin=lmin, lmax=lmax, **kw)
        u2, it2, res2, used2 = _native(D, b, base="block_jacobi", block=1, lmin=lmin, lmax=lmax, **kw)
        assert it1 == it2 > 0 and res1 == res2 and used1 == used2 and np.array_equal(u1.view(np.uint8), u2.view(np.uint8)), kw
    z1, z2 = _apply_gpu(D, b, "jacobi", 5, lmin, lmax), _apply_gpu(D, b, "block_jacobi", 5, lmin, lmax, block=1)
    assert np.all(np.isfinite(z1)) and np.array_equal(z1.view(np.uint8), z2.view(np.uint8))
    assert _lmax_gpu(D, "jacobi", 3, 16, b) == _lmax_gpu(D, "block_jacobi", 1, 16, b)
    D.close()


# ---- 2. beyond one trip of the grid ------------------------------------------------------------------------------
TRIP_CASES = [("none", 0, np.float64), ("none", 0, np.float32), ("jacobi", 0, np.float64), ("jacobi", 0, np.float32),
              ("block_jacobi", 2, np.float64), ("block_jacobi", 3, np.float64), ("block_jacobi", 4, np.float64)]


@pytest.mark.parametrize("base,bs,dtype", TRIP_CASES, ids=[f"{b}{s or ''}-{_f(d)}" for b, s, d in TRIP_CASES])
def test_beyond_one_grid_trip(base, bs, dtype):
    name = "band600001"
    P, A = _problem(name, dtype, base, block=bs or 3)
    assert P.n == 600001 and (bs == 0 or P.minv.shape[0] > 131072)
    b = _rhs(P.n, dtype)
    errors = _check_apply(name, P, A, dtype, bs or 3, (3,))
    errors += _iterates(name, P, A, b, dtype, bs or 3, 2, (1, 2))
    if base == "jacobi":  # degree 1: r . z comes from cheb_update_kernel itself
        errors += _iterates(name, P, A, b, dtype, bs or 3, 1, (1, 2))
    if base != "none":
        errors += _check_lmax(name, P, A, dtype, bs or 3, 4)
    A.close()
    assert not errors, f"{name} {base} {_f(dtype)}: " + "; ".join(errors)


def test_beyond_one_grid_trip_with_blocks_of_six():
    """133 334 blocks of six rows, the last one of five"""
    name, dtype = "band800003", np.float64
    P, A = _problem(name, dtype, "block_jacobi", block=6)
    assert P.minv.shape[0] == 133334 and P.n % 6 == 5
    errors = _check_apply(name, P, A, dtype, 6, (2,))
    A.close()
    assert not errors, "; ".join(errors)


# ---- 3. high degree ----------------------------------------------------------------------------------------------
def _bases(name):
    return ("none", "jacobi", "block_jacobi") if name.startswith("rand") else ("none", "jacobi")


@DTYPES
@pytest.mark.parametrize("name", ["rand1023", "pwtk@0.05"])
def test_high_degree_polynomial(name, dtype):
    errors, A = [], None
    for base in _bases(name):
        P, A = _problem(name, dtype, base, A)
        errors += _check_apply(name, P, A, dtype, 3, (8, 16))
    A.close()
    assert not errors, f"{name} {_f(dtype)}: " + "; ".join(errors)


@DTYPES
@pytest.mark.parametrize("name", ["rand1023", "pwtk@0.05"])
def test_high_degree_iterates(name, dtype):
    errors, A = [], None
    for base in _bases(name):
        P, A = _problem(name, dtype, base, A)
        b = _rhs(P.n, dtype)
        for m in (6, 16):
            errors += _iterates(name, P, A, b, dtype, 3, m, (1, 2, 3))
    A.close()
    assert not errors, f"{name} {_f(dtype)}: " + "; ".join(errors)


@DTYPES
def test_windows_at_high_degree(dtype):
    """m = 6: check_every = 1 / 3 / 1000 are windows of 1 / 3 / 4 iterations, m = 16: 1 / 1 / 1.  The iterations
    enqueued behind the converged one change neither u nor the count"""
    import cfs_spmv_amd as cfs
    n, rp, ci, va = _matrix("pwtk@0.05")
    va, b = scaled(n, rp, ci, va, dtype), _rhs(n, dtype)
    tol = 1e-8 if dtype == np.float64 else 1e-4
    D = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=DET))
    assert D.kernel_variant()["det"] == 1
    lmin, lmax = Problem(n, rp, ci, va, "jacobi").bounds()
    for m in (6, 16):
        kw = dict(degree=m, lmin=lmin, lmax=lmax, tol=tol, maxiter=500)
        u1, it1, res1, _ = _native(D, b, check_every=1, **kw)
        print(f"cheb-edges windows  {_f(dtype)} pwtk@0.05 jacobi m={m}: {it1} iterations, relres {res1:.3e}")
        assert 2 < it1 < 500 and res1 <= 10 * tol
        for check_every in (3, 1000):
            u2, it2, res2, _ = _native(D, b, check_every=check_every, **kw)
            assert it2 == it1 and res2 == res1 and np.array_equal(u2.view(np.uint8), u1.view(np.uint8)), (m, check_every, it1, it2)
    D.close()


# ---- 4. a first guess that is not zero -------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("name", ["rand257", "pwtk@0.05"])
def test_first_guess_not_zero(name, dtype):
    errors, A = [], None
    for base in _bases(name):
        P, A = _problem(name, dtype, base, A)
        b = _rhs(P.n, dtype)
        x0 = np.random.default_rng(P.n + 5).uniform(-1, 1, P.n).astype(dtype)
        errors += _iterates(name, P, A, b, dtype, 3, 3, (1, 2, 5), x0=x0, label=" (x0)")
    A.close()
    assert not errors, f"{name} {_f(dtype)}: " + "; ".join(errors)
