/*
 * field_ops.hpp -- mass, gradient and weak divergence of fields on a Domain's mesh (an option of this build: the reference
 * has no such operators).  They are the halves the stiffness operator is made of, A_L u = wdiv(grad u), run by the kernels of
 * csrc/fdd_field.hip, which form the metric J^-1 per point from the coordinates instead of reading it from arrays.
 *
 * What the kernels read beyond the Domain's own D_hat -- the coordinates of the points and the GLL weights -- is uploaded at
 * first use (3 x 8 B per point: 403 MB at 32^3 elements of degree 7) and freed with the Domain.  D_hat is the Domain's
 * current device table, so a set_D_hat is followed without further work.
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

// the three operators on device vectors of the Domain's points (element-local, unassembled); no output may be an input
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
};

} // namespace fdd

#endif
