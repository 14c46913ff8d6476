/*
 * lifetime_main.cpp -- TEST INFRASTRUCTURE.  Walks a problem of the host layer through everything that owns "device"
 * memory on the CPU stand-in, in one executable under AddressSanitizer (Makefile: _build/lifetime_asan), and counts what
 * the kernel library has handed out with fdd_live_objects.  A use after free, a double free or an out-of-bounds read of a
 * block is the sanitizer's report; a block, plan or graph that outlives its problem is a failed assertion here; a host
 * leak is the leak check's report at exit.  Uses include/fdd_host.h and fdd_live_objects only.
 */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fdd_hip.h"
#include "fdd_host.h"

namespace
{

struct Live
{
    long long v[6]; // blocks, bytes, peak bytes, plans, graphs, mallocs ever
};

Live live()
{
    Live l;
    if (fdd_live_objects(l.v, 6) != 0)
    {
        fprintf(stderr, "fdd_live_objects failed\n");
        exit(1);
    }
    return l;
}

#define OK(call)                                                                                  \
    do                                                                                            \
    {                                                                                             \
        if ((call) != 0)                                                                          \
        {                                                                                         \
            fprintf(stderr, "%s:%d: %s failed: %s\n", __FILE__, __LINE__, #call, fddh_last_error()); \
            exit(1);                                                                              \
        }                                                                                         \
    } while (0)

void require(bool ok, const char *what, const Live &a, const Live &b)
{
    if (ok) return;
    fprintf(stderr, "FAILED: %s: blocks %lld / %lld, bytes %lld / %lld, plans %lld / %lld, graphs %lld / %lld\n", what, a.v[0], b.v[0], a.v[1], b.v[1], a.v[3], b.v[3], a.v[4], b.v[4]);
    exit(1);
}

// blocks, bytes, plans and graphs (the peak and the count of calls ever only grow)
bool same(const Live &a, const Live &b) { return a.v[0] == b.v[0] and a.v[1] == b.v[1] and a.v[3] == b.v[3] and a.v[4] == b.v[4]; }

void solve(fddh_problem *p, const std::vector<double> &f, std::vector<double> &u)
{
    std::vector<double> hist(4096);
    int nh = 0, its = 0;
    OK(fddh_problem_solve(p, 0, f.data(), u.data(), hist.data(), (int)hist.size(), &nh, &its));
}

void walk(int flags, const Live &baseline)
{
    const int E[3] = {2, 2, 2}, P[3] = {1, 1, 1};
    fddh_problem *p = nullptr;
    OK(fddh_problem_create_box_ex(&p, E, P, 5, 2, 1, 1, flags));
    long long info[FDDH_INFO_COUNT];
    OK(fddh_problem_info(p, info, FDDH_INFO_COUNT));
    const int n = (int)info[FDDH_INFO_NUM_LOCAL_POINTS];
    const Live created = live();
    require(created.v[0] > baseline.v[0] and created.v[1] > baseline.v[1] and created.v[3] > baseline.v[3], "a created problem holds blocks and plans", created, baseline);

    int levels = 0;
    OK(fddh_problem_amg_build(p, 0, 0.0, 1, 0, &levels));
    const Live built = live();
    require(built.v[0] > created.v[0] and built.v[3] > created.v[3], "a hierarchy holds blocks and plans", built, created);

    OK(fddh_problem_set_options(p, 50, 1.0e-8, -1, -1, -1, -1, -1, -1));
    std::vector<double> u_star(n), f(n), u(n);
    OK(fddh_problem_make_rhs(p, 0, 1, u_star.data(), f.data()));
    solve(p, f, u);

    // a new diffusivity rebuilds the hierarchy: the old one goes, so every setting leaves what the first left
    std::vector<double> kappa(n);
    Live first{};
    const bool conforming = (flags & FDDH_FORCE_COMPOSITE) == 0; // a composite region refuses a diffusivity
    for (int k = 0; conforming and k < 3; k++)
    {
        for (int q = 0; q < n; q++) kappa[q] = 1.0 + 0.25 * k + 0.5 * ((q * 7 + k) % 5);
        OK(fddh_diffusivity_set(p, kappa.data(), n));
        const Live now = live();
        if (k == 0) first = now;
        require(same(now, first), "a rebuilt hierarchy replaces the one before it", now, first);
        require(now.v[5] > built.v[5], "the rebuild allocated", now, built);
    }
    for (int k = 0; not conforming and k < 3; k++) // there the Chebyshev order of the V-cycle's smoother rebuilds it
    {
        OK(fddh_problem_set_flag(p, "amg_cheby_order", k == 1 ? 2 : 3));
        const Live now = live();
        if (k == 0) first = now;
        require(same(now, first), "a rebuilt hierarchy replaces the one before it", now, first);
        require(now.v[5] > built.v[5], "the rebuild allocated", now, built);
    }
    solve(p, f, u);
    if (conforming) OK(fddh_diffusivity_set(p, nullptr, 0));

    OK(fddh_problem_set_flag(p, "preconditioner_precision", 32)); // the float inner solve
    solve(p, f, u);
    OK(fddh_problem_set_flag(p, "preconditioner_precision", 64));
    {
        OK(fddh_problem_set_flag(p, "sub_use_preconditioner", 2)); // point-Jacobi: what the Chebyshev-Jacobi inner solve runs with
        OK(fddh_problem_set_flag(p, "inner_solver", 1));
        solve(p, f, u);
        OK(fddh_problem_set_flag(p, "preconditioner_precision", 32));
        solve(p, f, u);
        OK(fddh_problem_set_flag(p, "preconditioner_precision", 64));
        OK(fddh_problem_set_flag(p, "inner_solver", 0));
        OK(fddh_problem_set_flag(p, "sub_use_preconditioner", 1));
    }

    int degree = 0;
    OK(fddh_problem_level_degree(p, 0, &degree));
    std::vector<double> D((size_t)(degree + 1) * (degree + 1));
    OK(fddh_problem_get_D_hat(p, 0, D.data(), degree + 1));
    OK(fddh_problem_set_D_hat(p, 0, D.data(), degree + 1));
    double last = 0.0;
    OK(fddh_problem_pcg_begin(p, f.data()));
    OK(fddh_problem_pcg_steps(p, 5, &last));
    OK(fddh_problem_pcg_solution(p, u.data()));

    OK(fddh_problem_projection_configure(p, 4));
    {
        std::vector<double> hist(4096);
        int nh = 0, its = 0;
        double proj[4], seconds = 0.0;
        OK(fddh_problem_solve_projected(p, 0, f.data(), u.data(), hist.data(), (int)hist.size(), &nh, &its, proj, &seconds));
    }

    const Live before = live();
    OK(fddh_problem_destroy(p));
    const Live after = live();
    require(before.v[0] > built.v[0], "the solves took buffers of their own", before, built);
    require(same(after, baseline), "a destroyed problem gives everything back", after, baseline);
}

} // namespace

int main()
{
    OK(fddh_init(0, nullptr, 0));
    OK(fddh_comm_single());
    OK(fddh_set_print(0));
    const Live baseline = live();
    for (int round = 0; round < 2; round++)
    {
        walk(FDDH_WITH_SUBDOMAIN, baseline);
        walk(FDDH_WITH_SUBDOMAIN | FDDH_FORCE_COMPOSITE, baseline);
    }
    OK(fddh_rank_finalize());
    printf("ok\n");
    return 0;
}
