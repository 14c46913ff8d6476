// Prints the host layer's stiffness kernel choice (host/element_operator.hpp) for every reachable combination of list state,
// flags, precision and form, one row each; tests/test_cpu_stiffness_choice.py builds it against the CPU stand-in of the
// kernel library and holds every row to tests/stiffness_choice_rules.py.  The flags are written into the struct directly:
// the stand-in lacks the optional entries, so the setter would refuse most of them.
// row: dim degree affine offdiag_zero shared_blocks lean64 lean32 | the six flags | f32 form in_place |
//      family shared lean label bytes_per_point | info: diag mfma_diag lines shared lean
#include <cstdio>

#include "element_operator.hpp"

int main()
{
    using namespace fdd;
    const char *family_name[] = {"two_launch", "fused_2d", "fused", "diag", "lines", "mfma", "mfma_diag", "affine", "mfma_affine"};
    const int degrees[] = {1, 2, 3, 5, 7, 8, 11, 15, 16};
    for (int dim = 2; dim <= 3; dim++)
        for (int degree : degrees)
            for (int state = 0; state < 32; state++)
            {
                LevelList ll;
                ll.dim = dim, ll.poly_degree = degree, ll.num_elements = 8;
                ll.affine = state & 1, ll.offdiag_zero = state & 2, ll.shared_blocks = state & 4, ll.lean_D_hat = state & 8, ll.lean_D_hat32 = state & 16;
                // the reachable states (LevelList)
                const bool fused_3d = dim == 3 and degree <= 15;
                if (((ll.affine or ll.offdiag_zero) and not fused_3d) or (ll.shared_blocks and not ll.offdiag_zero) or ((ll.lean_D_hat or ll.lean_D_hat32) and degree != 7)) continue;
                for (int bits = 0; bits < 64; bits++)
                {
                    StiffnessFlags flags;
                    flags.mfma_stiffness = bits & 1, flags.skip_zero_factors = bits & 2, flags.line_stiffness = bits & 4;
                    flags.mfma_skip_zero_factors = bits & 8, flags.shared_factor_blocks = bits & 16, flags.lean_line_stiffness = bits & 32;
                    for (int which = 0; which < 4; which++) // local, local in place, gather in double, gather in float
                    {
                        const bool f32 = which == 3, in_place = which == 1;
                        const StiffnessForm form = which < 2 ? StiffnessForm::local : StiffnessForm::gather;
                        const StiffnessChoice c = choose_stiffness(ll, flags, f32, form, in_place);
                        const StiffnessProfile p = stiffness_profile(form, c, f32);
                        const StiffnessChoice g = choose_stiffness(ll, flags, f32, StiffnessForm::gather);
                        printf("%d %d %d %d %d %d %d | %d %d %d %d %d %d | %d %s %d | %s %d %d %s %g | %d %d %d %d %d\n", dim, degree, (int)ll.affine, (int)ll.offdiag_zero, (int)ll.shared_blocks, (int)ll.lean_D_hat, (int)ll.lean_D_hat32,
                               (int)flags.mfma_stiffness, (int)flags.skip_zero_factors, (int)flags.line_stiffness, (int)flags.mfma_skip_zero_factors, (int)flags.shared_factor_blocks, (int)flags.lean_line_stiffness,
                               (int)f32, which < 2 ? "local" : "gather", (int)in_place, family_name[(int)c.family], (int)c.shared, (int)c.lean, p.label ? p.label : "-", p.bytes_per_point,
                               (int)g.three_arrays(), (int)g.mfma_three_arrays(), (int)g.lines(), (int)g.shared_lines(), (int)g.lean_lines());
                    }
                }
            }
    return 0;
}
