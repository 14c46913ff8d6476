/*
 * helmholtz.hpp -- the zeroth-order term of -laplace(u) + lambda u -- a LABELLED OPTION of this build (the reference solves
 * the Poisson problem), the counterpart of diffusivity.hpp.
 *
 * lambda is a constant or one double per point of the fine level, finite and >= 0.  The term is the vector
 *
 *     c[n] = sum over the copies p of node n of lambda_p B_p       B: the diagonal mass matrix (fdd_field_mass)
 *
 * which Domain::set_shift sums from the products this file forms and the node-space outer loops add behind the gather; the
 * Subdomain keeps the same values in its own dof numbering (Subdomain::set_shift), for Subdomain::operator_dofs.
 *
 * What this file holds: the checks of a caller's lambda, the products, and the map of the node vector into dofs.  Which
 * solve carries the term is said where the solves start (helmholtz_inner_refusal, helmholtz_outer_refusal in
 * fdd_host_capi.cpp; Subdomain::helmholtz_refusal).
 */
#ifndef FDD_HELMHOLTZ_HPP
#define FDD_HELMHOLTZ_HPP

#include <cmath>
#include <string>
#include <vector>

#include "diffusivity.hpp"

namespace fdd
{
namespace helmholtz
{

// Why a lambda (lambda_points == nullptr: the constant) cannot be set on a problem of num_points fine-level points, or "":
// nothing is touched before this has passed.  missing_entry: the first kernel entry the term needs that the loaded library
// lacks; sub_points: the points the Subdomain covers, or -1 without one.  The first offending point is named.
inline std::string refusal(const char *missing_entry, int ranks, int dim, int poly_degree, bool composite, long long sub_points, double lambda, const double *lambda_points, long long num_points)
{
    using diffusivity::formatted;
    if (missing_entry) return formatted("a Helmholtz shift needs %s, which the loaded kernel library does not export", missing_entry);
    if (ranks > 1) return formatted("a Helmholtz shift is supported on one rank: this communicator has %d", ranks);
    if (dim != 3) return formatted("a Helmholtz shift is 3-D only: this problem is %d-D", dim);
    if (poly_degree > 15) return formatted("a Helmholtz shift supports poly_degree 1..15, got %d", poly_degree);
    if (composite) return "a Helmholtz shift needs a conforming region: this problem's Subdomain is a composite";
    if (sub_points >= 0 and sub_points != num_points) return "a Helmholtz shift needs a Subdomain over the rank's own points";
    for (long long q = 0; lambda_points and q < num_points; q++)
        if (not std::isfinite(lambda_points[q]) or lambda_points[q] < 0.0) return formatted("lambda must be finite and >= 0 at every point: point %zu has %g", (size_t)q, lambda_points[q]);
    if (not lambda_points and (not std::isfinite(lambda) or lambda < 0.0)) return formatted("lambda must be finite and >= 0, got %g", lambda);
    return "";
}

// mass[q] (B_q on entry) becomes lambda_q B_q: one IEEE double product per point
inline void scale_mass(std::vector<double> &mass, double lambda, const double *lambda_points)
{
    for (size_t q = 0; q < mass.size(); q++) mass[q] = (lambda_points ? lambda_points[q] : lambda) * mass[q];
}

// the node vector c in a Subdomain's dof numbering: a dof sits on the node of any of its points
inline std::vector<double> dofs_of_nodes(const std::vector<double> &c_nodes, const int *point_node, const int *point_dof, size_t num_points, int num_dofs)
{
    std::vector<double> c_dofs((size_t)num_dofs, 0.0);
    for (size_t q = 0; q < num_points; q++)
        if (point_dof[q] >= 0 and point_dof[q] < num_dofs) c_dofs[point_dof[q]] = c_nodes[point_node[q]];
    return c_dofs;
}

} // namespace helmholtz
} // namespace fdd

#endif
