/*
 * field_ops.hpp -- mass, gradient and weak divergence of fields on a Domain's mesh (an option of this build: the reference
 * has no such operators).  They are the halves the stiffness operator is made of, A_L u = wdiv(grad u), run by the kernels of
 * csrc/fdd_field.hip, which form the metric J^-1 per point from the coordinates instead of reading it from arrays.
 *
 * What the kernels read beyond the Domain's own D_hat -- the coordinates of the points and the GLL weights -- is uploaded at
 * first use (3 x 8 B per point: 403 MB at 32^3 elements of degree 7) and freed with the Domain.  D_hat is the Domain's
 * current device table, so a set_D_hat is followed without further work.
 *
 * The convection term c . grad u (fdd_field_convect, fdd_field_weak_convect) comes with the tables of its quadrature: the
 * M = (3n+1)/2 Gauss-Legendre points and weights, the interpolation P from the GLL points to them and P' = P D_hat.  P' is
 * made from the Domain's current host table and made again when that has changed, so it follows a set_D_hat as D_hat does.
 */
#ifndef FDD_FIELD_OPS_HPP
#define FDD_FIELD_OPS_HPP

#include <stdexcept>
#include <string>
#include <vector>

#include "fdd_device.hpp"
#include "gll.hpp"

namespace fdd
{

// the device copy of mesh.x / y / z and of the GLL weights; a member of Domain
struct FieldGeometry
{
    memory xyz[3];
    memory weights;
    bool uploaded = false;

    FieldGeometry() {}
    FieldGeometry(const FieldGeometry &) = delete;
    FieldGeometry &operator=(const FieldGeometry &) = delete;

    template <typename Mesh>
    void upload(const Mesh &mesh, int poly_degree)
    {
        if (uploaded) return;
        const int n = poly_degree + 1;
        const std::vector<double> *c[3] = {&mesh.x, &mesh.y, &mesh.z};
        for (int a = 0; a < 3; a++)
        {
            xyz[a] = dev().malloc<double>(c[a]->size());
            xyz[a].copyFrom(c[a]->data(), c[a]->size() * sizeof(double));
        }
        std::vector<double> z(n), w(n);
        gll::zwgll(z.data(), w.data(), n);
        weights = dev().malloc<double>(n);
        weights.copyFrom(w.data(), n * sizeof(double));
        uploaded = true;
    }

    // the quadrature of the over-integrated convection term on the host: z, w (M), P and Pd (M x n, row q at q n)
    int num_quad = 0;
    std::vector<double> quad_z, quad_w, P_hst, Pd_hst;
    std::vector<double> Pd_table;    // the D_hat that Pd_hst was made from
    memory P, Pd, quad_weights;      // the device copies of P_hst, Pd_hst and quad_w, made at the first weak_convect
    std::vector<double> Pd_uploaded; // the D_hat that the device copy of Pd was made from; empty: nothing is uploaded yet

    void quadrature(const std::vector<double> &D_hat, int poly_degree)
    {
        const int n = poly_degree + 1;
        if (num_quad == 0)
        {
            const int M = (3 * n + 1) / 2;
            std::vector<double> z(n), w(n);
            gll::zwgll(z.data(), w.data(), n);
            quad_z.resize(M);
            quad_w.resize(M);
            gll::zwgl(quad_z.data(), quad_w.data(), M);
            P_hst = gll::interpolation_matrix(z.data(), n, quad_z.data(), M);
            num_quad = M;
        }
        if (Pd_table != D_hat)
        {
            Pd_hst.assign((size_t)num_quad * n, 0.0);
            for (int q = 0; q < num_quad; q++)
                for (int p = 0; p < n; p++)
                    for (int i = 0; i < n; i++) Pd_hst[(size_t)q * n + i] += P_hst[(size_t)q * n + p] * D_hat[(size_t)p * n + i]; // D[p][i]
            Pd_table = D_hat;
        }
    }

    void upload_quadrature(const std::vector<double> &D_hat, int poly_degree)
    {
        quadrature(D_hat, poly_degree);
        const size_t bytes = P_hst.size() * sizeof(double);
        if (Pd_uploaded.empty())
        {
            P = dev().malloc<double>(P_hst.size());
            P.copyFrom(P_hst.data(), bytes);
            Pd = dev().malloc<double>(P_hst.size());
            quad_weights = dev().malloc<double>(num_quad);
            quad_weights.copyFrom(quad_w.data(), num_quad * sizeof(double));
        }
        if (Pd_uploaded != Pd_table)
        {
            Pd.copyFrom(Pd_hst.data(), bytes);
            Pd_uploaded = Pd_table;
        }
    }
};

// why the field operators cannot run on this Domain with the loaded kernel library, or empty
template <typename Dom>
std::string field_refusal(const Dom &d)
{
    if (const char *missing = missing_field_entry()) return std::string("the field operators need ") + missing + ", which the loaded kernel library does not export";
    if (d.mesh.dim != 3) return "the field operators are 3-D only: this problem is " + std::to_string(d.mesh.dim) + "-D";
    if (d.poly_degree < 1 or d.poly_degree > 15) return "the field operators support poly_degree 1..15, got " + std::to_string(d.poly_degree);
    return std::string();
}

// the operators on device vectors of the Domain's points (element-local, unassembled); no output may be an input
template <typename Dom>
struct FieldOps
{
    Dom &d;
    const double *X[3];

    explicit FieldOps(Dom &domain) : d(domain)
    {
        const std::string why = field_refusal(d);
        if (!why.empty()) throw std::runtime_error(why);
        d.field_geometry.upload(d.mesh, d.poly_degree);
        for (int a = 0; a < 3; a++) X[a] = d.field_geometry.xyz[a].template as<double>();
    }

    const double *D_hat() const { return d.D_hat.template as<double>(); }
    const double *weights() const { return d.field_geometry.weights.template as<double>(); }

    void mass(memory &out) const { FDD_CALL(fdd_field_mass(out.as<double>(), X, D_hat(), weights(), d.num_local_elements, d.poly_degree, dev().stream)); }

    void gradient(memory &gx, memory &gy, memory &gz, const memory &u) const
    {
        double *const g[3] = {gx.as<double>(), gy.as<double>(), gz.as<double>()};
        FDD_CALL(fdd_field_gradient(g, u.as<double>(), X, D_hat(), d.num_local_elements, d.poly_degree, dev().stream));
    }

    void weak_divergence(memory &out, const memory &vx, const memory &vy, const memory &vz) const
    {
        const double *const v[3] = {vx.as<double>(), vy.as<double>(), vz.as<double>()};
        FDD_CALL(fdd_field_weak_divergence(out.as<double>(), v, X, D_hat(), weights(), d.num_local_elements, d.poly_degree, dev().stream));
    }

    // c . grad u at the points
    void convect(memory &out, const memory &cx, const memory &cy, const memory &cz, const memory &u) const
    {
        const double *const c[3] = {cx.as<double>(), cy.as<double>(), cz.as<double>()};
        FDD_CALL(fdd_field_convect(out.as<double>(), c, u.as<double>(), X, D_hat(), d.num_local_elements, d.poly_degree, dev().stream));
    }

    // out_i = integral of phi_i (c . grad u) on the (3n+1)/2 Gauss points, unassembled
    void weak_convect(memory &out, const memory &cx, const memory &cy, const memory &cz, const memory &u) const
    {
        FieldGeometry &g = d.field_geometry;
        g.upload_quadrature(d.D_hat_hst, d.poly_degree);
        const double *const c[3] = {cx.as<double>(), cy.as<double>(), cz.as<double>()};
        FDD_CALL(fdd_field_weak_convect(out.as<double>(), c, u.as<double>(), X, D_hat(), g.P.template as<double>(), g.Pd.template as<double>(), g.quad_weights.template as<double>(), g.num_quad, d.num_local_elements, d.poly_degree,
                                        dev().stream));
    }
};

} // namespace fdd

#endif
