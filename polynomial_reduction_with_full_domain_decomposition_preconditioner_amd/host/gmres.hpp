/*
 * gmres.hpp -- the host recurrence of flexible GMRES(m), stated once: the reference has it twice (domain.tpp:727-914,
 * subdomain.tpp:4309-4489) and the restructured, node-space and dof-space forms of this build repeat it.  Here are the
 * Hessenberg matrix with its Givens rotations (GmresScalars) and the restart loop (gmres_solve); the vectors -- where
 * they live, which kernels work on them, what is timed -- belong to the caller, who hands them in as a GmresSpace.
 * The device-bookkeeping inner solve (Subdomain::gmres_dofs_device_t) keeps these numbers in the one-thread kernels of
 * csrc/fdd_krylov.hip and does not come through here; neither does the oracle, which is the checker.
 */
#ifndef FDD_GMRES_HPP
#define FDD_GMRES_HPP

#include <cmath>
#include <functional>
#include <vector>

namespace fdd
{

// H, the rotations (c, s) and the rotated right-hand side gamma of one solve.  Nothing survives from one solve to the
// next: every entry a step reads was written earlier in the same cycle, so resize() at the start of a solve is all the
// sizing there is, and it allocates only when m has changed.  After back_substitute, c holds the update's coefficients (as the reference's c_gmres does).
template <typename DType>
struct GmresScalars
{
    std::vector<std::vector<DType>> H;
    std::vector<DType> c, s, gamma;

    void resize(int m)
    {
        if ((int)H.size() == m and (int)gamma.size() == m + 1) return; // stale entries are never read
        H.assign(m, std::vector<DType>(m, 0.0));
        c.assign(m, 0.0);
        s.assign(m, 0.0);
        gamma.assign(m + 1, 0.0);
    }

    // Column j of H holds the Gram-Schmidt coefficients, alpha_j = |q|: apply the earlier rotations to the column, form
    // the new one and advance gamma (domain.tpp:824-850).  False when alpha_j == 0 (the Krylov space is exhausted;
    // nothing past the column's rotation is done), otherwise r_norm = |gamma[j + 1]|.
    bool rotate(int j, DType alpha_j, DType &r_norm)
    {
        for (int i = 0; i < j; i++)
        {
            DType h_ij = H[i][j];
            H[i][j] = c[i] * h_ij + s[i] * H[i + 1][j];
            H[i + 1][j] = -s[i] * h_ij + c[i] * H[i + 1][j];
        }
        if (std::abs(alpha_j) == 0.0) return false;

        const DType beta_j = std::sqrt(H[j][j] * H[j][j] + alpha_j * alpha_j);
        const DType gamma_j = 1.0 / beta_j;
        c[j] = H[j][j] * gamma_j;
        s[j] = alpha_j * gamma_j;
        H[j][j] = beta_j;
        gamma[j + 1] = -s[j] * gamma[j];
        gamma[j] = c[j] * gamma[j];
        r_norm = std::abs(gamma[j + 1]);
        return true;
    }

    // back substitution over columns 0..j, stored into c (domain.tpp:891-899)
    void back_substitute(int j)
    {
        for (int k = j; k >= 0; k--)
        {
            DType gamma_k = gamma[k];
            for (int i = j; i > k; i--) gamma_k -= H[k][i] * c[i];
            c[k] = gamma_k / H[k][k];
        }
    }
};

// The stopping rules, and the two places where the reference's Domain and Subdomain loops are not the same loop.
template <typename DType>
struct GmresControl
{
    int max_iterations;
    DType tolerance;
    bool use_relative; // test r_norm / r_0_norm instead of r_norm

    // Subdomain counts a step when it starts (subdomain.tpp:4370), Domain when it has made v_{j+1} (domain.tpp:886), and
    // both test `iter >= max_iterations` in between: with a cap that is not a multiple of m the Domain loop runs one
    // step more.  The step number printed is the same either way.
    bool count_at_step_start;

    // Domain leaves the loop on a NaN residual (domain.tpp:876-880); Subdomain has no such test and runs to its cap.
    bool stop_on_nan;
};

// The vector work of one solve: the caller assigns a lambda over its own vectors to each member by name.
template <typename DType>
struct GmresSpace
{
    std::function<DType()> initial_norm;                                      // |r_0| of the initial iterate
    std::function<DType()> restart_norm;                                      // r = f - A u for the current iterate, and |r|
    std::function<void(DType)> start_cycle;                                   // v_0 = r / gamma_0
    std::function<DType(int, std::vector<std::vector<DType>> &)> arnoldi_step; // z_j = M^-1 v_j, q = A z_j, H[0..j][j] = <q, v_i>, q -= sum H[i][j] v_i; returns alpha_j = |q|
    std::function<void(int, DType)> next_vector;                              // v_{j+1} = q / alpha_j
    std::function<void(int, const std::vector<DType> &)> add_update;          // u += sum_{i <= j} c[i] z_i
};

// Flexible GMRES(m) from a zero (or the caller's) initial iterate.  Pushes |r_0| and every step's residual norm onto
// `history`, reports each through print(step, r_norm, r_norm / r_0_norm) -- the third difference between the two
// classes: Domain prints "Iter %2d" on rank 0, Subdomain "- Iter %3d" to the rank's log -- and returns the step count
// (Domain assigns it to num_iterations, domain.tpp:913; Subdomain adds it, subdomain.tpp:4488).
template <typename DType, typename Print>
int gmres_solve(GmresScalars<DType> &g, int m, const GmresControl<DType> &ctl, const GmresSpace<DType> &space, std::vector<DType> &history, Print print)
{
    g.resize(m);
    const DType r_0_norm = space.initial_norm();
    history.push_back(r_0_norm);
    print(0, r_0_norm, (DType)1.0);

    bool converged = false;
    int iter = 0, j;
    while (iter < ctl.max_iterations)
    {
        g.gamma[0] = (iter > 0) ? space.restart_norm() : r_0_norm;
        space.start_cycle(g.gamma[0]);

        for (j = 0; j < m; j++)
        {
            if (ctl.count_at_step_start) iter++;

            const DType alpha_j = space.arnoldi_step(j, g.H);
            DType r_norm;
            if (not g.rotate(j, alpha_j, r_norm))
            {
                converged = true;
                break;
            }
            history.push_back(r_norm);
            print(ctl.count_at_step_start ? iter : iter + 1, r_norm, r_norm / r_0_norm);

            // hitting max_iterations counts as converged (domain.tpp:870-874, subdomain.tpp:4449-4453)
            if ((ctl.use_relative ? r_norm / r_0_norm : r_norm) < ctl.tolerance or iter >= ctl.max_iterations or (ctl.stop_on_nan and std::isnan(r_norm)))
            {
                converged = true;
                break;
            }

            space.next_vector(j, alpha_j);
            if (not ctl.count_at_step_start) iter++;
        }

        if (j == m) j--;
        g.back_substitute(j);
        space.add_update(j, g.c);

        if (converged) break;
    }
    return iter;
}

} // namespace fdd

#endif
