// C-ABI over the C++ host classes (include/fdd_host.h).  Everything here is
// plumbing: it instantiates Domain<double> / Subdomain<double> the way the
// reference's run_simulation does (poisson.cpp:150-251) and moves host vectors
// in and out of device memory.
#include "fdd_host.h"

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstring>
#include <limits>
#include <exception>
#include <memory>
#include <string>
#include <sys/stat.h>
#include <unordered_map>
#include <functional>
#include <vector>

#include "boundary.hpp"
#include "box_mesh.hpp"
#include "domain.hpp"
#include "field_ops.hpp"
#include "helmholtz.hpp"
#include "subdomain.hpp"

typedef double SType; // config.hpp:19 STYPE
typedef double PType; // config.hpp:20 PTYPE (AMG/config.hpp:4 Float)

static thread_local char g_err[512] = "";

static int fail(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return -1;
}

struct fddh_problem
{
    int poly_degree = 1;
    int poly_reduction = 1;
    std::vector<int> degrees; // N, N-r, ..., 1
    std::unordered_map<int, Domain<SType>> domains;
    std::unique_ptr<Subdomain<PType>> subdomain; // declared after `domains`, so destroyed first: its lists view the Domain's factor arrays
    NoPreconditioner none;

    // The rank (= host thread) that built the problem: its device stream, communicator and globals are thread_local, so a
    // call from any other thread would silently run on the legacy default stream with a one-rank communicator (every
    // collective skipped: wrong sums, or peers hanging in RCCL).  Every fddh_problem_* entry checks it first (on_problem).
    unsigned long long owner = 0; // device_t::rank_instance of that rank; never 0 for a finished problem

    // device staging vectors
    fdd::memory a, b, c;
    fdd::memory sa, sb; // subdomain-sized

    double helmholtz_min = 0.0, helmholtz_max = 0.0; // of the lambda a set Helmholtz shift was made from (fddh_helmholtz_set)
    double diffusivity_min = 0.0, diffusivity_max = 0.0; // of the kappa that is set (fddh_diffusivity_set; 0: none)

    // The two terms the shift is rebuilt from (rebuild_shift), per point of the fine level, each empty while it is off: the
    // products lambda_q B_q of a set Helmholtz shift and the sums r[q] of a set Robin coefficient (boundary.hpp)
    std::vector<double> lambda_B, robin_r;
    double robin_min = 0.0, robin_max = 0.0; // of the alpha that is set (fddh_boundary_robin_set; 0: none)
    // a generated mesh: its spec (the face codes among it) and the faces of the rank's elements on the surface of the box,
    // on the host and, from the first fddh_boundary_surface on, on the device.  A problem made from files has neither
    bool generated = false;
    fdd::BoxSpec spec;
    fdd::boundary::FaceList faces;
    fdd::memory face_elem_dev, face_side_dev;

    Domain<SType> &fine() { return domains[poly_degree]; }
    const Domain<SType> &fine() const { return domains.at(poly_degree); }
};

// identity of the calling rank: unique over the life of the process, 0 on a thread that is not (or no longer) a rank
static unsigned long long this_rank() { return fdd::dev().rank_instance; }
static std::atomic<unsigned long long> rank_instances{0};

// 0 when the calling thread is an initialised rank (fddh_init) and, for a problem, the one that built it
static int rank_check(const fddh_problem *p = nullptr)
{
    if (!fdd::dev().initialised) return fail("fddh_init has not been called on this thread: the host layer's device stream and communicator are per rank = per host thread");
    if (p && (p->owner == 0 || p->owner != this_rank())) return fail("this problem was built by another rank (host thread); its stream and communicator are not the calling thread's");
    return 0;
}

namespace
{

// the frame of every entry: what the body returns, or -1 with the text of what it threw
template <typename Body>
int guarded(Body &&body)
{
    try
    {
        return body();
    }
    catch (const std::exception &e)
    {
        return fail("%s", e.what());
    }
}

// The opening of a fddh_problem_* entry, in this order: the calling thread is the problem's rank (rank_check); the problem
// and the pointers the entry cannot do without are there (args_ok, which is formed before the rank is known and so must not
// look into *p; refused with `refusal`); then the body on *p.  A test that needs *p is the body's own
template <typename Problem, typename Body>
int on_problem(Problem *p, bool args_ok, const char *refusal, Body &&body)
{
    return guarded([&] {
        if (int rc = rank_check(p)) return rc;
        if (!p || !args_ok) return fail("%s", refusal);
        return body(*p);
    });
}

template <typename Problem, typename Body>
int on_problem(Problem *p, bool args_ok, Body &&body)
{
    return on_problem(p, args_ok, "null argument", body);
}

// the same for an entry that is about the Subdomain: the body gets *p and *p->subdomain
template <typename Problem, typename Body>
int on_subdomain(Problem *p, bool args_ok, Body &&body)
{
    return on_problem(p, args_ok, [&](Problem &pr) {
        if (!pr.subdomain) return fail("problem was created without a Subdomain");
        return body(pr, *pr.subdomain);
    });
}

// the same for the fddh_field_* entries: the body gets *p and the field operators of its fine Domain, whose constructor
// throws what they cannot run on (a kernel library without their entries, a 2-D problem: field_ops.hpp)
template <typename Body>
int on_field_ops(fddh_problem *p, bool args_ok, Body &&body)
{
    return on_problem(p, args_ok, [&](fddh_problem &pr) { return body(pr, fdd::FieldOps<Domain<SType>>(pr.fine())); });
}

size_t fine_bytes(const fddh_problem &p) { return (size_t)p.fine().num_local_points * sizeof(double); }

// the two forms of the convection term (fddh_convect, fddh_weak_convect): c and u in through p.a, p.b, p.c and a fourth vector,
// the result out of a fifth
template <typename Op>
int convect_entry(fddh_problem *p, const double *cx, const double *cy, const double *cz, const double *u, double *out, Op &&op)
{
    return on_problem(p, cx && cy && cz && u && out, [&](fddh_problem &pr) {
        if (const char *missing = fdd::missing_convect_entry()) return fail("the convection operators need %s, which the loaded kernel library does not export", missing);
        const fdd::FieldOps<Domain<SType>> ops(pr.fine());
        fdd::memory field = fdd::dev().malloc<double>(pr.fine().num_local_points), result = fdd::dev().malloc<double>(pr.fine().num_local_points);
        pr.a.copyFrom(cx, fine_bytes(pr));
        pr.b.copyFrom(cy, fine_bytes(pr));
        pr.c.copyFrom(cz, fine_bytes(pr));
        field.copyFrom(u, fine_bytes(pr));
        op(ops, result, pr.a, pr.b, pr.c, field);
        result.copyTo(out, fine_bytes(pr));
        return 0;
    });
}

// a vector of the fine level's points in through p.a, op, its result out through p.b (out may be null: the result stays in p.b)
template <typename Op>
void fine_round_trip(fddh_problem &p, const double *in, double *out, Op &&op)
{
    p.a.copyFrom(in, fine_bytes(p));
    op();
    if (out) p.b.copyTo(out, fine_bytes(p));
}

// its counterpart for the Subdomain's vectors: in through p.sa, out through p.sb
size_t sub_bytes(const fddh_problem &p) { return (size_t)p.subdomain->num_values * sizeof(double); }

template <typename Op>
void sub_round_trip(fddh_problem &p, const double *in, double *out, Op &&op)
{
    p.sa.copyFrom(in, sub_bytes(p));
    op();
    p.sb.copyTo(out, sub_bytes(p));
}

template <typename T>
void copy_history(const std::vector<T> &h, double *history, int history_cap, int *num_history)
{
    const int nh = (int)h.size();
    if (history)
        for (int i = 0; i < nh && i < history_cap; i++) history[i] = h[i];
    if (num_history) *num_history = nh;
}

// an entry that is about to run the inner solve: why the Chebyshev-Jacobi option cannot run on this problem as it is
// configured (the flags may be set in any order, so this is looked at when a solve starts), or nullptr
const char *inner_solver_refusal(const fddh_problem &p)
{
    if (!p.subdomain || !p.subdomain->chebyshev()) return nullptr;
    return p.subdomain->chebyshev_refusal();
}

// the same for an outer solve, which runs the inner one where the preconditioner is in use
const char *outer_solve_refusal(const fddh_problem &p)
{
    return p.subdomain && p.fine().use_preconditioner ? inner_solver_refusal(p) : nullptr;
}

// f(the problem's Subdomain) or f(no preconditioner): the callers differ in the test that chooses
template <typename F>
auto with_preconditioner(fddh_problem &p, bool use_subdomain, F &&f)
{
    if (use_subdomain) return f(*p.subdomain);
    return f(p.none);
}

// With a Helmholtz shift set (fddh_helmholtz_set): why a solve would not carry it, or nullptr.  The term lives in the
// node-space outer loops and in Subdomain::operator_dofs and nowhere else, so whatever would run another loop is refused
// when it starts (the flags may be set in any order).  inner: the inner solve alone (inner_fcg: called as the inner FCG);
// outer_gmres: the outer GMRES, else FCG
const char *helmholtz_inner_refusal(fddh_problem &p, bool inner_fcg = false)
{
    if (!p.fine().shift_active() || !p.subdomain) return nullptr;
    if (const char *why = p.subdomain->helmholtz_refusal()) return why;
    return inner_fcg ? "a Helmholtz shift needs the inner GMRES or Chebyshev-Jacobi in dof space: the inner FCG does not go through operator_dofs" : nullptr;
}

// Every face natural and no zeroth-order term: the operator has the constants in its null space, and a solve would converge
// in the residual to a solution that is off by a constant (the V-cycle returns values of no meaning).  Creating such a problem
// is allowed, because a shift may follow; what would solve with it is refused when it starts.
const char *singular_refusal(fddh_problem &p)
{
    if (!p.generated || p.fine().shift_active()) return nullptr;
    for (char c : p.spec.faces)
        if (c == 'D') return nullptr;
    return "this problem is singular: every face is natural ('N') and no zeroth-order term is set, so the constants are in the operator's null space; give it a 'D' face, a Helmholtz shift (fddh_helmholtz_set) or a Robin coefficient (fddh_boundary_robin_set)";
}

const char *helmholtz_outer_refusal(fddh_problem &p, bool outer_gmres)
{
    Domain<SType> &d = p.fine();
    if (!d.shift_active()) return nullptr;
    const bool nodes = with_preconditioner(p, p.subdomain != nullptr, [&](auto &preconditioner) { return d.can_fcg_nodes(preconditioner); });
    if (!nodes || (outer_gmres && !d.restructured_outer)) return "a Helmholtz shift needs the node-space outer solve (assembled_outer_solve = 1, restructured_inner_solve = 1, the inner GMRES or Chebyshev-Jacobi in dof space): the point-space outer loops do not carry the term";
    return d.use_preconditioner ? helmholtz_inner_refusal(p) : nullptr;
}

// ---- an operator change: every entry that changes the operator of a live problem ends here ----
// What hangs on the operator: (1) the projection basis and its images; in the Subdomain (2) the host copy of a level's table,
// the lists' lean verdicts and the float table, (3) the exact Jacobi diagonal, its two inverses, the Chebyshev bound
// cheby.lambda and operator_generation, with it the first step's scaling ChebyVectors::w, (4) the per-list verdicts, float
// copies and coefficient members, (5) a hierarchy that amg_build made (one that was handed in is the caller's and stays).
// (4) is read from arrays only kappa rewrites and is made again where they are rewritten (Domain::set_diffusivity,
// Subdomain::set_diffusivity); the rest is emptied here, by what changed:
struct OperatorChange
{
    enum Kind
    {
        table,      // a level's D_hat: (1) (2) (3).  The low-order matrix is assembled from the mesh, not from D_hat: (5) stays
        arithmetic, // the element kernels' arithmetic (affine_geometry): (1) (3).  The values move by rounding only: (5) stays
        shift,      // the Helmholtz term: (1) (3) (5), the term sits on the diagonal of the level-0 matrix.  A shift that was and stays off changes nothing
        factors     // the factor arrays (kappa): (1) (3) (5), kappa scales the level-0 matrix
    } kind;
    int degree = -1; // table: the level's degree, the table, its size
    const double *D = nullptr;
    int n = 0;
    bool was_active = false; // shift: was one set before the call

    static OperatorChange of_table(int degree, const double *D, int n) { return {table, degree, D, n}; }
    static OperatorChange of_shift(bool was_active) { return {shift, -1, nullptr, 0, was_active}; }
};

static void operator_changed(fddh_problem &p, const OperatorChange &c)
{
    Domain<SType> &d = p.fine();
    if (c.kind == OperatorChange::shift && !c.was_active && !d.shift_active()) return;
    d.projection.clear(); // (1): the basis and its images belong to the operator as it was
    if (!p.subdomain) return;
    const char *low_order_term = nullptr; // (5): what the printed line says was set or cleared
    if (c.kind == OperatorChange::shift) low_order_term = d.shift_active() ? "Helmholtz shift set" : "Helmholtz shift cleared";
    if (c.kind == OperatorChange::factors) low_order_term = d.diffusivity_active() ? "diffusivity set" : "diffusivity cleared";
    p.subdomain->operator_changed(c.degree, c.D, c.n, low_order_term); // (2) where a table is given, (3) always
}

// fn() between finish + barrier (collective: every rank or none) and finish, the wall time into *seconds; seconds null: fn() alone
template <typename Fn>
void wall_timed(double *seconds, Fn &&fn)
{
    std::chrono::steady_clock::time_point t0;
    if (seconds)
    {
        fdd::dev().finish();
        fdd::comm().barrier();
        t0 = std::chrono::steady_clock::now();
    }
    fn();
    if (seconds)
    {
        fdd::dev().finish();
        *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
}

// What the outer solve entries share: the inner solver's refusal, f staged in, run(fine Domain, preconditioner) with the
// problem's Subdomain or none -- from p.a into p.b, timed where seconds is given --, then u (where asked for) and the history out
template <typename Run>
int outer_solve(fddh_problem &p, const double *f, double *u, double *history, int history_cap, int *num_history, int *num_iterations, double *seconds, Run &&run)
{
    if (const char *why = outer_solve_refusal(p)) return fail("%s", why);
    if (const char *why = singular_refusal(p)) return fail("%s", why);
    Domain<SType> &d = p.fine();
    fine_round_trip(p, f, u, [&] {
        wall_timed(seconds, [&] { with_preconditioner(p, p.subdomain != nullptr, [&](auto &preconditioner) { run(d, preconditioner); }); });
    });
    copy_history(d.residual_history, history, history_cap, num_history);
    if (num_iterations) *num_iterations = d.num_iterations;
    return 0;
}

// solver_id 0: flexible CG, else GMRES(m)
template <typename Preconditioner>
void krylov_solve(fddh_problem &p, Domain<SType> &d, Preconditioner &preconditioner, int solver_id)
{
    if (solver_id == 0)
        d.flexible_conjugate_gradient(p.b, p.a, preconditioner);
    else
        d.generalized_minimum_residual(p.b, p.a, preconditioner);
}

} // namespace

static std::vector<int> level_degrees(int N, int reduction)
{
    std::vector<int> d;
    d.push_back(N);
    while (d.back() > 1)
    {
        int r = d.back() - reduction;
        d.push_back(r >= 1 ? r : 1);
    }
    return d;
}

// FDD_SETUP_TIMING=1: rank 0 prints the host time of the setup's parts
static double setup_clock() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static void setup_lap(const char *what, int degree, double &mark)
{
    static const bool on = getenv("FDD_SETUP_TIMING") != nullptr;
    const double t = setup_clock();
    if (on and fdd::comm().rank == 0) printf("setup: %-28s N = %-2d %8.3f s\n", what, degree, t - mark);
    mark = t;
}

static void finish_problem(fddh_problem *p, int flags, int sub_overlap, int sup_overlap)
{
    double mark = setup_clock();
    p->owner = this_rank();
    const int with_subdomain = flags & FDDH_WITH_SUBDOMAIN;
    Domain<SType> &dom = p->fine();
    p->a = fdd::dev().malloc<double>(dom.num_local_points);
    p->b = fdd::dev().malloc<double>(dom.num_local_points);
    p->c = fdd::dev().malloc<double>(dom.num_local_points);
    if (with_subdomain)
    {
        rstdout("Setting up subdomain object...\n");
        p->subdomain.reset(new Subdomain<PType>());
        p->subdomain->block_local = (flags & FDDH_BLOCK_LOCAL) != 0;
        p->subdomain->force_composite = (flags & FDDH_FORCE_COMPOSITE) != 0;
        p->subdomain->initialize(p->domains, p->poly_degree, p->poly_reduction, sub_overlap, sup_overlap);
        setup_lap("Subdomain::initialize", p->poly_degree, mark);
        p->sa = fdd::dev().malloc<double>(p->subdomain->num_values);
        p->sb = fdd::dev().malloc<double>(p->subdomain->num_values);
        dom.use_preconditioner = true;
    }
    else
    {
        dom.use_preconditioner = false;
    }
}

// fddh_comm_callbacks and _ex: the latter also needs, and hands on, exchange_bytes
static int comm_callbacks(int rank, int size, void *ctx, fddh_allreduce_fn allreduce_sum_f64, fddh_allreduce_fn allreduce_max_f64, fddh_allgather_fn allgather_bytes, fddh_barrier_fn barrier, fddh_exchange_fn exchange_bytes, bool with_exchange)
{
    return guarded([&] {
        if (int rc = rank_check()) return rc;
        if (rank < 0 || size < 1 || rank >= size || !allreduce_sum_f64 || !allreduce_max_f64 || !allgather_bytes || !barrier || (with_exchange && !exchange_bytes)) return fail("bad callback set");
        fdd::CommCallbacks cb;
        cb.ctx = ctx;
        cb.allreduce_sum_f64 = allreduce_sum_f64;
        cb.allreduce_max_f64 = allreduce_max_f64;
        cb.allgather_bytes = allgather_bytes;
        cb.barrier = barrier;
        cb.exchange_bytes = exchange_bytes;
        fdd::set_comm(new fdd::CallbackComm(rank, size, cb));
        fdd::globals().proc_id = rank;
        fdd::globals().num_procs = size;
        return 0;
    });
}

// `iterations` launches of y = A x in milliseconds, timed with events on the stream after three launches to warm up
static float spmv_ms(CSR_Matrix<SType> &A, fdd::memory &x, fdd::memory &y, int iterations)
{
    void *e0 = nullptr, *e1 = nullptr;
    FDD_CALL(fdd_event_create(&e0));
    FDD_CALL(fdd_event_create(&e1));
    for (int i = 0; i < 3; i++) A.multiply(y, x);
    FDD_CALL(fdd_event_record(e0, fdd::dev().stream));
    for (int i = 0; i < iterations; i++) A.multiply(y, x);
    FDD_CALL(fdd_event_record(e1, fdd::dev().stream));
    float ms = 0.0f;
    FDD_CALL(fdd_event_elapsed_ms(&ms, e0, e1));
    FDD_CALL(fdd_event_destroy(e0));
    FDD_CALL(fdd_event_destroy(e1));
    return ms;
}

extern "C" {

const char *fddh_last_error(void) { return g_err; }

int fddh_init(int device, void *stream, int own_stream)
{
    return guarded([&] {
        if (fdd_set_device(device) != 0) return fail("fdd_set_device(%d): %s", device, fdd_last_error());
        if (own_stream)
        {
            void *s = nullptr;
            if (fdd_stream_create(&s) != 0) return fail("fdd_stream_create: %s", fdd_last_error());
            stream = s;
        }
        fdd::dev().owns_stream = own_stream != 0;
        fdd::dev().stream = stream;
        if (!fdd::dev().initialised) fdd::dev().rank_instance = ++rank_instances; // a further fddh_init of a live rank changes its stream, not who it is
        fdd::dev().initialised = true;
        return 0;
    });
}

int fddh_set_print(int on)
{
    return guarded([&] {
        fdd::globals().print = on != 0;
        return 0;
    });
}

int fddh_set_timer(int on)
{
    return guarded([&] {
        fdd_timer().enabled = on != 0;
        if (on) fdd_timer().initialize();
        return 0;
    });
}

int fddh_timer_total(const char *key, double *seconds)
{
    return guarded([&] {
        if (!key || !seconds) return fail("null argument");
        *seconds = fdd_timer().total(key);
        return 0;
    });
}

int fddh_timer_total_over_ranks(const char *key, const char *aggregation, double *seconds)
{
    return guarded([&] {
        if (!key || !aggregation || !seconds) return fail("null argument");
        *seconds = fdd_timer().total(key, aggregation); // collective: all-reduce (max or sum) over the ranks, timer.tpp:67
        return 0;
    });
}

int fddh_comm_single(void)
{
    return guarded([&] {
        if (int rc = rank_check()) return rc;
        fdd::set_comm(new fdd::SingleComm());
        fdd::globals().proc_id = 0;
        fdd::globals().num_procs = 1;
        return 0;
    });
}

int fddh_local_world_create(void **world, int size)
{
    return guarded([&] {
        if (!world || size < 1) return fail("bad argument");
        *world = new std::shared_ptr<fdd::LocalWorld>(new fdd::LocalWorld(size));
        return 0;
    });
}

int fddh_local_world_destroy(void *world)
{
    delete static_cast<std::shared_ptr<fdd::LocalWorld> *>(world);
    return 0;
}

int fddh_local_world_fail(void *world)
{
    return guarded([&] {
        if (!world) return fail("null argument");
        (*static_cast<std::shared_ptr<fdd::LocalWorld> *>(world))->fail();
        return 0;
    });
}

int fddh_rank_finalize(void)
{
    return guarded([&] {
        fdd::device_t &d = fdd::dev();
        if (!d.initialised) return 0;
        if (d.stream) fdd_stream_sync(d.stream);
        fdd::set_comm(new fdd::SingleComm()); // deletes the thread's communicator (and its device scratch)
        if (d.owns_stream && d.stream) fdd_stream_destroy(d.stream);
        d.stream = nullptr;
        d.owns_stream = false;
        d.initialised = false;
        d.rank_instance = 0; // the problems this rank built are nobody's now: every entry refuses them
        return 0;
    });
}

int fddh_comm_local(void *world, int rank)
{
    return guarded([&] {
        if (int rc = rank_check()) return rc;
        if (!world) return fail("null argument");
        std::shared_ptr<fdd::LocalWorld> w = *static_cast<std::shared_ptr<fdd::LocalWorld> *>(world);
        if (rank < 0 || rank >= w->size) return fail("bad rank");
        fdd::set_comm(new fdd::LocalComm(w, rank));
        fdd::globals().proc_id = rank;
        fdd::globals().num_procs = w->size;
        return 0;
    });
}

int fddh_comm_rccl_unique_id(char *out128)
{
    return guarded([&] {
        if (!out128) return fail("null argument");
        fdd::RcclComm tmp;
        tmp.unique_id(out128);
        return 0;
    });
}

int fddh_comm_rccl_init(const char *id128, int rank, int size)
{
    return guarded([&] {
        if (int rc = rank_check()) return rc;
        if (!id128 || rank < 0 || size < 1 || rank >= size) return fail("bad rank/size");
        fdd::RcclComm *c = new fdd::RcclComm();
        c->init(id128, rank, size);
        fdd::set_comm(c);
        fdd::globals().proc_id = rank;
        fdd::globals().num_procs = size;
        return 0;
    });
}

int fddh_comm_callbacks(int rank, int size, void *ctx, fddh_allreduce_fn allreduce_sum_f64, fddh_allreduce_fn allreduce_max_f64, fddh_allgather_fn allgather_bytes, fddh_barrier_fn barrier)
{
    return comm_callbacks(rank, size, ctx, allreduce_sum_f64, allreduce_max_f64, allgather_bytes, barrier, nullptr, false);
}

int fddh_comm_callbacks_ex(int rank, int size, void *ctx, fddh_allreduce_fn allreduce_sum_f64, fddh_allreduce_fn allreduce_max_f64, fddh_allgather_fn allgather_bytes, fddh_barrier_fn barrier, fddh_exchange_fn exchange_bytes)
{
    return comm_callbacks(rank, size, ctx, allreduce_sum_f64, allreduce_max_f64, allgather_bytes, barrier, exchange_bytes, true);
}

// Drives every collective of the active communicator once, bypassing the
// "size == 1" shortcuts of the solver, and checks the results.
int fddh_comm_selftest(int n)
{
    return guarded([&] {
        if (int rc = rank_check()) return rc;
        if (n < 1) return fail("n must be positive");
        fdd::Comm &c = fdd::comm();
        const int R = c.size, me = c.rank;
        std::vector<double> h(n);
        for (int i = 0; i < n; i++) h[i] = (double)(me + 1) * (i + 1);
        fdd::memory d = fdd::dev().malloc<double>(n);
        fdd::memory g = fdd::dev().malloc<double>((size_t)n * R);

        d.copyFrom(h.data(), n * sizeof(double));
        c.allreduce_sum(d.as<double>(), n);
        std::vector<double> out(n);
        d.copyTo(out.data(), n * sizeof(double));
        const double tri = 0.5 * R * (R + 1);
        for (int i = 0; i < n; i++)
            if (out[i] != tri * (i + 1)) return fail("allreduce_sum: element %d is %g, expected %g", i, out[i], tri * (i + 1));

        d.copyFrom(h.data(), n * sizeof(double));
        c.allreduce_max(d.as<double>(), n);
        d.copyTo(out.data(), n * sizeof(double));
        for (int i = 0; i < n; i++)
            if (out[i] != (double)R * (i + 1)) return fail("allreduce_max: element %d is %g", i, out[i]);

        d.copyFrom(h.data(), n * sizeof(double));
        c.allgather(d.ptr(), g.ptr(), n * sizeof(double));
        std::vector<double> all((size_t)n * R);
        g.copyTo(all.data(), all.size() * sizeof(double));
        for (int p = 0; p < R; p++)
            for (int i = 0; i < n; i++)
                if (all[(size_t)p * n + i] != (double)(p + 1) * (i + 1)) return fail("allgather: rank %d element %d is %g", p, i, all[(size_t)p * n + i]);

        std::vector<long long> mine(me + 2, 100 + me);
        std::vector<int> counts;
        std::vector<long long> cat = c.allgatherv_host(mine, counts);
        size_t expect = 0;
        for (int p = 0; p < R; p++) expect += p + 2;
        if (cat.size() != expect) return fail("allgatherv_host: %zu entries, expected %zu", cat.size(), expect);

        // point-to-point: every rank sends (me + 1) * (i + 1) + 1000 * peer to its two ring neighbours (one message per
        // peer and direction, as the composite's ring pull does), on device buffers and through the host helper
        if (R > 1)
        {
            const int left = (me + R - 1) % R, right = (me + 1) % R;
            std::vector<int> peers;
            peers.push_back(right);
            if (left != right) peers.push_back(left);
            std::vector<fdd::memory> sb(peers.size()), rb(peers.size());
            std::vector<fdd::ExchangeOp> ops(peers.size());
            for (size_t k = 0; k < peers.size(); k++)
            {
                const int ns = n + peers[k], nr = n + me; // sizes differ per direction
                for (int i = 0; i < n; i++) h[i] = (double)(me + 1) * (i + 1) + 1000.0 * peers[k];
                std::vector<double> msg(ns, -1.0);
                std::copy(h.begin(), h.end(), msg.begin());
                sb[k] = fdd::dev().malloc<double>(ns);
                rb[k] = fdd::dev().malloc<double>(nr);
                sb[k].copyFrom(msg.data(), ns * sizeof(double));
                ops[k].peer = peers[k];
                ops[k].send = sb[k].ptr();
                ops[k].send_bytes = ns * sizeof(double);
                ops[k].recv = rb[k].ptr();
                ops[k].recv_bytes = nr * sizeof(double);
            }
            c.exchange(ops.data(), (int)ops.size());
            for (size_t k = 0; k < peers.size(); k++)
            {
                std::vector<double> got(n + me);
                rb[k].copyTo(got.data(), got.size() * sizeof(double));
                for (int i = 0; i < n; i++)
                    if (got[i] != (double)(peers[k] + 1) * (i + 1) + 1000.0 * me) return fail("exchange: element %d from rank %d is %g", i, peers[k], got[i]);
            }
            std::vector<std::vector<char>> out(R);
            for (int p = 0; p < R; p++) out[p].assign((size_t)(3 + me + 2 * p), (char)(17 * me + p));
            std::vector<std::vector<char>> in = c.exchange_host(out);
            for (int p = 0; p < R; p++)
            {
                if (in[p].size() != (size_t)(3 + p + 2 * me)) return fail("exchange_host: %zu bytes from rank %d", in[p].size(), p);
                for (char ch : in[p])
                    if (ch != (char)(17 * p + me)) return fail("exchange_host: wrong payload from rank %d", p);
            }
        }

        c.barrier();
        return 0;
    });
}

int fddh_comm_info(int *rank, int *size, char *name, size_t name_len)
{
    return guarded([&] {
        if (int rc = rank_check()) return rc;
        if (rank) *rank = fdd::comm().rank;
        if (size) *size = fdd::comm().size;
        if (name && name_len) snprintf(name, name_len, "%s", fdd::comm().name());
        return 0;
    });
}

int fddh_problem_create_box(fddh_problem **out, const int E[3], const int P[3], int poly_degree, int poly_reduction, int with_subdomain)
{
    return fddh_problem_create_box_ex(out, E, P, poly_degree, poly_reduction, 1, 1, with_subdomain ? FDDH_WITH_SUBDOMAIN : 0);
}

int fddh_problem_create_box_ex(fddh_problem **out, const int E[3], const int P[3], int poly_degree, int poly_reduction, int subdomain_overlap, int superdomain_overlap, int flags)
{
    return fddh_problem_create_kershaw_ex(out, E, P, poly_degree, poly_reduction, subdomain_overlap, superdomain_overlap, flags, 1.0, 1.0);
}

int fddh_problem_create_kershaw_ex(fddh_problem **out, const int E[3], const int P[3], int poly_degree, int poly_reduction, int subdomain_overlap, int superdomain_overlap, int flags, double eps_y, double eps_z)
{
    return fddh_problem_create_box_faces(out, E, P, poly_degree, poly_reduction, subdomain_overlap, superdomain_overlap, flags, eps_y, eps_z, "DDDDDD");
}

int fddh_problem_create_box_faces(fddh_problem **out, const int E[3], const int P[3], int poly_degree, int poly_reduction, int subdomain_overlap, int superdomain_overlap, int flags, double eps_y, double eps_z, const char *faces)
{
    return guarded([&] {
        if (int rc = rank_check()) return rc;
        const std::string bad_faces = fdd::boundary::faces_refusal(faces);
        if (!bad_faces.empty()) return fail("%s", bad_faces.c_str());
        if (!(eps_y > 0.0 && eps_y <= 1.0 && eps_z > 0.0 && eps_z <= 1.0)) return fail("Kershaw eps must lie in (0, 1]");
        const int with_subdomain = flags & FDDH_WITH_SUBDOMAIN;
        if (!out || !E || !P || poly_degree < 1 || poly_reduction < 1) return fail("bad argument");
        if (P[0] * P[1] * P[2] != fdd::comm().size) return fail("rank grid %dx%dx%d does not match communicator size %d", P[0], P[1], P[2], fdd::comm().size);
        for (int d = 0; d < 3; d++)
            if (E[d] < 1 || P[d] < 1 || E[d] % P[d] != 0) return fail("elements per direction must be a multiple of the rank blocks");

        fddh_problem *p = new fddh_problem();
        p->poly_degree = poly_degree;
        p->poly_reduction = poly_reduction;
        p->degrees = with_subdomain ? level_degrees(poly_degree, poly_reduction) : std::vector<int>(1, poly_degree);

        fdd::BoxSpec spec;
        for (int d = 0; d < 3; d++)
        {
            spec.E[d] = E[d];
            spec.P[d] = P[d];
        }
        spec.kershaw_eps[0] = eps_y;
        spec.kershaw_eps[1] = eps_z;
        memcpy(spec.faces, faces, 6);
        p->generated = true;
        p->spec = spec;
        p->faces = fdd::boundary::box_faces(spec, fdd::comm().rank);

        for (int deg : p->degrees)
        {
            rstdout("Setting up domain \"N = %d\" object...\n", deg);
            double mark = setup_clock();
            MeshData<SType> mesh = fdd::make_box_mesh<SType>(spec, deg, fdd::comm().rank);
            setup_lap("box mesh", deg, mark);
            p->domains[deg].initialize(std::move(mesh));
            setup_lap("Domain::initialize", deg, mark);
        }
        // `dim` follows the last mesh read in the reference; keep the fine one current
        fdd::globals().dim = p->fine().mesh.dim;

        finish_problem(p, flags, subdomain_overlap, superdomain_overlap);
        *out = p;
        return 0;
    });
}

int fddh_problem_create_dir(fddh_problem **out, const char *directory, int poly_degree, int poly_reduction, int subdomain_overlap, int superdomain_overlap, int with_subdomain)
{
    return fddh_problem_create_dir_ex(out, directory, poly_degree, poly_reduction, subdomain_overlap, superdomain_overlap, with_subdomain ? FDDH_WITH_SUBDOMAIN : 0);
}

int fddh_problem_create_dir_ex(fddh_problem **out, const char *directory, int poly_degree, int poly_reduction, int subdomain_overlap, int superdomain_overlap, int flags)
{
    return guarded([&] {
        if (int rc = rank_check()) return rc;
        const int with_subdomain = flags & FDDH_WITH_SUBDOMAIN;
        if (!out || !directory || poly_degree < 1 || poly_reduction < 1) return fail("bad argument");
        fddh_problem *p = new fddh_problem();
        p->poly_degree = poly_degree;
        p->poly_reduction = poly_reduction;
        p->degrees = with_subdomain ? level_degrees(poly_degree, poly_reduction) : std::vector<int>(1, poly_degree);
        for (int deg : p->degrees)
        {
            MeshData<SType> m;
            if (!Domain<SType>::read_mesh_files(directory, deg, fdd::comm().rank, m))
            {
                delete p;
                return fail("cannot read mesh files of degree %d for rank %d under '%s'", deg, fdd::comm().rank, directory);
            }
            rstdout("Setting up domain \"N = %d\" object...\n", deg);
            p->domains[deg].initialize(std::move(m));
        }
        fdd::globals().dim = p->fine().mesh.dim;
        finish_problem(p, flags, subdomain_overlap, superdomain_overlap);
        *out = p;
        return 0;
    });
}

int fddh_problem_destroy(fddh_problem *p)
{
    return guarded([&] {
        if (int rc = rank_check(p)) return rc;
        delete p; // every member owns what it holds
        return 0;
    });
}

int fddh_write_box_mesh_files(const char *directory, const int E[3], const int P[3], int poly_degree, int rank)
{
    return fddh_write_kershaw_mesh_files(directory, E, P, poly_degree, rank, 1.0, 1.0);
}

int fddh_write_kershaw_mesh_files(const char *directory, const int E[3], const int P[3], int poly_degree, int rank, double eps_y, double eps_z)
{
    return fddh_write_box_faces_mesh_files(directory, E, P, poly_degree, rank, eps_y, eps_z, "DDDDDD");
}

int fddh_write_box_faces_mesh_files(const char *directory, const int E[3], const int P[3], int poly_degree, int rank, double eps_y, double eps_z, const char *faces)
{
    return guarded([&] {
        if (!directory || !E || !P) return fail("null argument");
        const std::string bad_faces = fdd::boundary::faces_refusal(faces);
        if (!bad_faces.empty()) return fail("%s", bad_faces.c_str());
        if (!(eps_y > 0.0 && eps_y <= 1.0 && eps_z > 0.0 && eps_z <= 1.0)) return fail("Kershaw eps must lie in (0, 1]");
        fdd::BoxSpec spec;
        for (int d = 0; d < 3; d++)
        {
            spec.E[d] = E[d];
            spec.P[d] = P[d];
        }
        spec.kershaw_eps[0] = eps_y;
        spec.kershaw_eps[1] = eps_z;
        memcpy(spec.faces, faces, 6);
        MeshData<SType> m = fdd::make_box_mesh<SType>(spec, poly_degree, rank);
        char sub[4096];
        mkdir(directory, 0777);
        snprintf(sub, sizeof(sub), "%s/lx1_%d", directory, poly_degree + 1);
        mkdir(sub, 0777);
        if (!Domain<SType>::write_mesh_files(directory, rank, m)) return fail("cannot write mesh files under '%s'", directory);
        return 0;
    });
}

int fddh_problem_info(const fddh_problem *p, long long *info, int n)
{
    return on_problem(p, info != nullptr, [&](const fddh_problem &pr) {
        const Domain<SType> &d = pr.fine();
        long long v[FDDH_INFO_COUNT];
        v[FDDH_INFO_NUM_LOCAL_POINTS] = d.num_local_points;
        v[FDDH_INFO_NUM_LOCAL_NODES] = d.num_local_nodes;
        v[FDDH_INFO_NUM_BDARY_NODES] = d.boundary_nodes_count();
        v[FDDH_INFO_NUM_INTERFACE_SLOTS] = d.interface_slots_count();
        v[FDDH_INFO_NUM_TOTAL_NODES] = d.num_total_nodes;
        v[FDDH_INFO_NUM_TOTAL_ELEMENTS] = d.num_total_elements;
        v[FDDH_INFO_NUM_LOCAL_ELEMENTS] = d.num_local_elements;
        v[FDDH_INFO_NUM_LEVELS] = (long long)pr.degrees.size();
        v[FDDH_INFO_SUB_NUM_VALUES] = pr.subdomain ? pr.subdomain->num_values : 0;
        v[FDDH_INFO_SUB_NUM_DOFS] = pr.subdomain ? pr.subdomain->dofs() : 0;
        v[FDDH_INFO_NUM_ITERATIONS] = d.num_iterations;
        v[FDDH_INFO_DIM] = d.mesh.dim;
        for (int i = 0; i < n && i < FDDH_INFO_COUNT; i++) info[i] = v[i];
        return 0;
    });
}

int fddh_problem_sub_info(const fddh_problem *p, long long *info, int n)
{
    return on_subdomain(p, info != nullptr, [&](const fddh_problem &pr, const Subdomain<PType> &s) {
        const fdd::composite::Composite &c = s.composite_description();
        long long v[FDDH_SUB_INFO_COUNT];
        const int own_elems = pr.fine().num_local_elements, own_pts = pr.fine().num_local_points;
        v[FDDH_SUB_IS_COMPOSITE] = s.composite() ? 1 : 0;
        v[FDDH_SUB_NUM_ELEMS] = s.composite() ? c.num_sub_elems : own_elems;
        v[FDDH_SUB_NUM_EXT_ELEMS] = s.composite() ? c.num_sub_ext_elems : own_elems;
        v[FDDH_SUB_NUM_POINTS] = s.composite() ? c.num_sub_ext_points : own_pts;
        v[FDDH_SUB_NUM_SUB_DOFS] = s.composite() ? c.sub_num_dofs : s.dofs();
        v[FDDH_SUB_NUM_SUB_EXT_DOFS] = s.composite() ? c.sub_num_ext_dofs : s.dofs();
        v[FDDH_SUB_NUM_INTERFACE_DOFS] = s.composite() ? c.num_interface_dofs : 0;
        v[FDDH_SUB_NUM_SUP_DOFS] = s.composite() ? c.sup_num_dofs : 0;
        v[FDDH_SUB_NUM_SUP_EXT_DOFS] = s.composite() ? c.sup_num_ext_dofs : 0;
        v[FDDH_SUB_NUM_UNIQUE_DOFS] = s.dofs();
        v[FDDH_SUB_NUM_COARSE_DOFS] = s.composite() ? c.num_coarse_dofs : 0;
        v[FDDH_SUB_NUM_VALUES] = s.num_values;
        v[FDDH_SUB_OWN_POINTS] = own_pts;
        v[FDDH_SUB_NUM_PEERS] = s.composite() ? (long long)c.peers.size() : 0;
        for (int i = 0; i < n && i < FDDH_SUB_INFO_COUNT; i++) info[i] = v[i];
        return 0;
    });
}

int fddh_problem_sub_region(const fddh_problem *p, int *element, int *level, int n)
{
    return on_subdomain(p, element && level, [&](const fddh_problem &, const Subdomain<PType> &s) {
        if (!s.composite()) return fail("the region is the rank's own elements (no composite)");
        const fdd::composite::Composite &c = s.composite_description();
        if (n != c.num_sub_ext_elems) return fail("the region has %d elements", c.num_sub_ext_elems);
        for (int r = 0; r < n; r++)
        {
            element[r] = c.sub[r].id;
            level[r] = c.sub[r].level;
        }
        return 0;
    });
}

int fddh_problem_sub_composite_levels(const fddh_problem *p, int *kept, int n, int *num_levels)
{
    return on_subdomain(p, num_levels != nullptr, [&](const fddh_problem &, const Subdomain<PType> &s) {
        const fdd::composite::Composite &c = s.composite_description();
        *num_levels = (int)c.comp_levels.size();
        for (int i = 0; i < n && i < *num_levels && kept; i++) kept[i] = c.comp_levels[i];
        return 0;
    });
}

int fddh_problem_level_degree(const fddh_problem *p, int level, int *poly_degree)
{
    return on_problem(p, poly_degree != nullptr, "bad level", [&](const fddh_problem &pr) {
        if (level < 0 || level >= (int)pr.degrees.size()) return fail("bad level");
        *poly_degree = pr.degrees[level];
        return 0;
    });
}

int fddh_problem_mesh_array(const fddh_problem *p, int level, const char *name, void *out, size_t bytes)
{
    return on_problem(p, name && out, "bad argument", [&](const fddh_problem &pr) {
        if (level < 0 || level >= (int)pr.degrees.size()) return fail("bad argument");
        const MeshData<SType> &m = pr.domains.at(pr.degrees[level]).mesh;
        const void *src = nullptr;
        size_t have = 0;
        std::string s(name);
        if (s == "x") { src = m.x.data(); have = m.x.size() * sizeof(SType); }
        else if (s == "y") { src = m.y.data(); have = m.y.size() * sizeof(SType); }
        else if (s == "z") { src = m.z.data(); have = m.z.size() * sizeof(SType); }
        else if (s == "glo_num") { src = m.glo_num.data(); have = m.glo_num.size() * sizeof(long long); }
        else if (s == "node_degree") { src = m.node_degree.data(); have = m.node_degree.size() * sizeof(int); }
        else if (s == "p_mask") { src = m.p_mask.data(); have = m.p_mask.size() * sizeof(SType); }
        else if (s.size() == 3 && s[0] == 'g' && s[1] == '_' && s[2] >= '1' && s[2] <= '6') { const int g = s[2] - '1'; src = m.g[g].data(); have = m.g[g].size() * sizeof(SType); }
        else return fail("unknown mesh array '%s'", name);
        if (bytes != have) return fail("mesh array '%s' has %zu bytes, caller gave %zu", name, have, bytes);
        memcpy(out, src, have);
        return 0;
    });
}

int fddh_problem_csr(const fddh_problem *p, int which, int *num_rows, int *num_cols, int *num_nnz, int *ptr, int *col, double *val)
{
    return on_problem(const_cast<fddh_problem *>(p), true, [&](fddh_problem &pr) {
        CSR_Matrix<SType> &A = (which == 0) ? pr.fine().scatter_matrix() : pr.fine().gather_matrix();
        if (num_rows) *num_rows = A.num_rows;
        if (num_cols) *num_cols = A.num_cols;
        if (num_nnz) *num_nnz = A.num_nnz;
        if (ptr) memcpy(ptr, A.ptr_hst.data(), A.ptr_hst.size() * sizeof(int));
        if (col) memcpy(col, A.col_hst.data(), A.col_hst.size() * sizeof(int));
        if (val) memcpy(val, A.val_hst.data(), A.val_hst.size() * sizeof(double));
        return 0;
    });
}

int fddh_problem_assembled_weight(const fddh_problem *p, double *out, int n)
{
    return on_problem(const_cast<fddh_problem *>(p), out != nullptr, [&](fddh_problem &pr) {
        if (n != pr.fine().num_local_nodes) return fail("assembled_weight has %d entries", pr.fine().num_local_nodes);
        pr.fine().assembled_weight_memory().copyTo(out, (size_t)n * sizeof(double));
        return 0;
    });
}

int fddh_problem_set_D_hat(fddh_problem *p, int level, const double *D_hat, int n)
{
    return on_problem(p, D_hat != nullptr, "bad argument", [&](fddh_problem &pr) {
        if (level < 0 || level >= (int)pr.degrees.size()) return fail("bad argument");
        if (n != pr.degrees[level] + 1) return fail("D_hat of level %d is %d x %d", level, pr.degrees[level] + 1, pr.degrees[level] + 1);
        pr.domains[pr.degrees[level]].set_D_hat(D_hat, n);
        operator_changed(pr, OperatorChange::of_table(pr.degrees[level], D_hat, n));
        return 0;
    });
}

int fddh_problem_get_D_hat(const fddh_problem *p, int level, double *D_hat, int n)
{
    return on_problem(p, D_hat != nullptr, "bad argument", [&](const fddh_problem &pr) {
        if (level < 0 || level >= (int)pr.degrees.size()) return fail("bad argument");
        if (n != pr.degrees[level] + 1) return fail("wrong size");
        const std::vector<double> &D = pr.domains.at(pr.degrees[level]).D_hat_hst;
        memcpy(D_hat, D.data(), D.size() * sizeof(double));
        return 0;
    });
}

int fddh_problem_set_options(fddh_problem *p, int max_iterations, double tolerance, int num_vectors, int use_preconditioner, int preconditioner_type, int sub_num_vectors, int sub_max_iterations, int sub_build_tree)
{
    return on_problem(p, true, [&](fddh_problem &pr) {
        Domain<SType> &d = pr.fine();
        if (max_iterations >= 0) d.max_iterations = max_iterations;
        if (!std::isnan(tolerance) && tolerance >= 0.0) d.tolerance = tolerance;
        if (num_vectors > 0) d.num_vectors = num_vectors;
        if (use_preconditioner >= 0)
        {
            if (use_preconditioner && !pr.subdomain) return fail("problem was created without a Subdomain");
            d.use_preconditioner = use_preconditioner != 0;
        }
        if (preconditioner_type >= 0) d.preconditioner_type = preconditioner_type;
        if (pr.subdomain)
        {
            if (sub_num_vectors > 0) pr.subdomain->num_vectors = sub_num_vectors;
            if (sub_max_iterations >= 0) pr.subdomain->max_iterations = sub_max_iterations;
            if (sub_build_tree >= 0) pr.subdomain->build_tree = sub_build_tree != 0;
        }
        return 0;
    });
}

int fddh_problem_affine_info(fddh_problem *p, int *fine_domain_affine, int *sub_lists_affine, int *sub_lists, double *max_deviation)
{
    return on_problem(p, true, [&](fddh_problem &pr) {
        Domain<SType> &dom = pr.fine();
        double worst = dom.operator_list().affine_deviation;
        int lists = 0, affine = 0;
        if (pr.subdomain)
            for (auto &ll : pr.subdomain->operator_lists())
            {
                lists++;
                if (ll.affine) affine++;
                worst = std::max(worst, ll.affine_deviation);
            }
        if (fine_domain_affine) *fine_domain_affine = dom.operator_list().affine ? 1 : 0;
        if (sub_lists_affine) *sub_lists_affine = affine;
        if (sub_lists) *sub_lists = lists;
        if (max_deviation) *max_deviation = worst;
        return 0;
    });
}

// what the five fddh_problem_*_info entries of the stiffness flags have in common: the flag, whether the fine Domain's list and
// how many of the Subdomain's lists run a kernel of its kind (the gather form's choice in the precision in use), and the
// number of lists.  more(list): what an entry reports beyond that, from the fine Domain's list
static int stiffness_info(fddh_problem *p, const char *flag, bool (fdd::StiffnessChoice::*is)() const, int *enabled, int *fine_domain, int *sub_lists_on, int *sub_lists, const std::function<void(const fdd::LevelList &)> &more = nullptr)
{
    return on_problem(p, true, [&](fddh_problem &pr) {
        Domain<SType> &dom = pr.fine();
        if (enabled) *enabled = fdd::stiffness_flag(dom.stiffness, flag) ? 1 : 0;
        if (fine_domain) *fine_domain = (dom.operator_choice().*is)() ? 1 : 0;
        if (more) more(dom.operator_list());
        if (sub_lists_on) *sub_lists_on = pr.subdomain ? pr.subdomain->count_lists(is) : 0;
        if (sub_lists) *sub_lists = pr.subdomain ? (int)pr.subdomain->operator_lists().size() : 0;
        return 0;
    });
}

int fddh_problem_zero_factor_info(fddh_problem *p, int *enabled, int *fine_domain_diag, int *sub_lists_diag, int *sub_lists)
{
    return stiffness_info(p, "skip_zero_factors", &fdd::StiffnessChoice::three_arrays, enabled, fine_domain_diag, sub_lists_diag, sub_lists);
}

int fddh_problem_mfma_zero_factor_info(fddh_problem *p, int *enabled, int *fine_domain_mfma_diag, int *sub_lists_mfma_diag, int *sub_lists)
{
    return stiffness_info(p, "mfma_skip_zero_factors", &fdd::StiffnessChoice::mfma_three_arrays, enabled, fine_domain_mfma_diag, sub_lists_mfma_diag, sub_lists);
}

int fddh_problem_line_stiffness_info(fddh_problem *p, int *enabled, int *fine_domain_lines, int *sub_lists_lines, int *sub_lists)
{
    return stiffness_info(p, "line_stiffness", &fdd::StiffnessChoice::lines, enabled, fine_domain_lines, sub_lists_lines, sub_lists);
}

int fddh_problem_shared_factor_info(fddh_problem *p, int *enabled, int *fine_domain_shared, int *fine_domain_classes, int *sub_lists_shared, int *sub_lists)
{
    return stiffness_info(p, "shared_factor_blocks", &fdd::StiffnessChoice::shared_lines, enabled, fine_domain_shared, sub_lists_shared, sub_lists, [&](const fdd::LevelList &list) {
        if (fine_domain_classes) *fine_domain_classes = list.factor_classes;
    });
}

int fddh_problem_lean_line_info(fddh_problem *p, int *enabled, int *fine_domain_table_ok, int *fine_domain_lean, int *sub_lists_lean, int *sub_lists)
{
    return stiffness_info(p, "lean_line_stiffness", &fdd::StiffnessChoice::lean_lines, enabled, fine_domain_lean, sub_lists_lean, sub_lists, [&](const fdd::LevelList &list) {
        if (fine_domain_table_ok) *fine_domain_table_ok = list.lean_D_hat ? 1 : 0;
    });
}

int fddh_problem_assembly_info(fddh_problem *p, int *enabled, int *in_effect, long long *rows, long long *points, int *reduced_row_blocks, char *why_not, size_t why_not_len)
{
    return on_subdomain(p, true, [&](fddh_problem &, Subdomain<PType> &sub) {
        if (enabled) *enabled = sub.stiffness.assemble_in_stiffness ? 1 : 0;
        const char *obstacle = sub.assembly_obstacle();
        if (!sub.assembly.built) sub.assembly_build(); // the classes are reported whether they are used or not
        if (in_effect) *in_effect = obstacle == nullptr ? 1 : 0;
        if (rows) std::copy(sub.assembly.rows, sub.assembly.rows + 3, rows);
        if (points) std::copy(sub.assembly.points, sub.assembly.points + 5, points);
        if (reduced_row_blocks) *reduced_row_blocks = sub.assembly.reduced_blocks;
        if (why_not && why_not_len > 0) snprintf(why_not, why_not_len, "%s", obstacle ? obstacle : "");
        return 0;
    });
}

int fddh_problem_assembly_arrays(fddh_problem *p, int *num_points, int *num_rows, int *num_nnz, int *point_class_dof, int *ptr, int *col, int *row_map)
{
    return on_subdomain(p, true, [&](fddh_problem &, Subdomain<PType> &sub) {
        if (!sub.assembly.built) sub.assembly_build();
        const fdd::AssemblyClasses &a = sub.assembly;
        if (!a.unusable.empty()) return fail("no classes: %s", a.unusable.c_str());
        if (num_points) *num_points = (int)a.point_class_dof.size();
        if (num_rows) *num_rows = (int)a.row_map.size();
        if (num_nnz) *num_nnz = (int)a.col.size();
        if (point_class_dof) std::copy(a.point_class_dof.begin(), a.point_class_dof.end(), point_class_dof);
        if (ptr) std::copy(a.ptr.begin(), a.ptr.end(), ptr);
        if (col) std::copy(a.col.begin(), a.col.end(), col);
        if (row_map) std::copy(a.row_map.begin(), a.row_map.end(), row_map);
        return 0;
    });
}

// ---- fddh_problem_set_flag ----
// Three tables, asked in this order: the flags that only switch a member on or off (here), the flags that choose between the
// stiffness kernels (fdd::stiffness_flag_row, element_operator.hpp) and the flags that check a range, need an entry of the
// kernel library, rebuild a hierarchy, clear the projection or refuse a problem without a Subdomain (coded_flag_row below).

// flag name -> the member it assigns `value != 0` to on every Domain (or none) and on the Subdomain (or none).  A row that
// only names a Subdomain member is accepted, and does nothing, on a problem without one
struct PlainFlagRow
{
    const char *name;
    bool Domain<SType>::*domain;
    bool Subdomain<PType>::*subdomain;
};

static const PlainFlagRow *plain_flag_row(const std::string &flag)
{
    typedef Domain<SType> D;
    typedef Subdomain<PType> S;
    static const PlainFlagRow table[] = {
        {"fused_dssum", &D::fused_dssum, &S::fused_dssum},
        {"restructured_inner_solve", &D::restructured_outer, &S::restructured}, // and the same restructure of the outer GMRES
        // gs_add on the boundary prefix as grouped sends / receives between the ranks that share nodes (default) or as
        // the dense interface-slot all-reduce; must be set alike on every rank
        {"neighbour_interface_exchange", &D::neighbour_interface_exchange, nullptr},
        // the coarse level's blocks inside the ring pull's group (default) or as an all-gather of their own; alike on every rank
        {"fold_coarse_exchange", nullptr, &S::fold_coarse_exchange},
        {"assembled_outer_solve", &D::assembled_outer, nullptr},
        {"shared_residual_norm", &D::shared_residual_norm, nullptr},
        {"skip_last_basis_store", nullptr, &S::skip_last_basis_store},
        {"early_gamma", &D::early_gamma, nullptr},
        {"unit_stitch_in_place", &D::unit_stitch_in_place, nullptr},
        {"fused_update_flexible_dot", &D::fused_update_flexible_dot, nullptr},
        // the outer step's passes that carry a neighbour's work (Domain::fcg_nodes_step_residual / _direction); each falls back
        // to the launches it replaces where the kernel library lacks its entry or its conditions do not hold
        {"fused_residual_norm", &D::fused_residual_norm, nullptr},
        {"solution_in_direction_pass", &D::solution_in_direction_pass, nullptr},
        {"lazy_steps", &D::lazy_steps, nullptr},
        {"device_bookkeeping", &D::device_scalars, &S::device_bookkeeping},
        {"assembled_inner_solve", nullptr, &S::assembled_inner},
    };
    for (const PlainFlagRow &row : table)
        if (flag == row.name) return &row;
    return nullptr;
}

// build the FEM matrix and the lattice levels of the AMG hierarchy in HBM (Subdomain::amg_build); needs the
// fdd_amg_setup_* entries of the kernel library
static int set_amg_device_setup(fddh_problem &p, const char *, int value)
{
    if (value != 0)
        if (const char *missing = fdd::missing_amg_setup_entry()) return fail("amg_device_setup needs %s, which the loaded kernel library does not export", missing);
    p.subdomain->amg_device_setup = value != 0;
    return 0;
}

static int set_sub_use_preconditioner(fddh_problem &p, const char *, int value)
{
    p.subdomain->use_preconditioner = value == 1;
    p.subdomain->use_jacobi = value == 2;
    return 0;
}

// an option of this build: elements that are affine images of the reference cube do not stream their factor
// arrays (element_operator.hpp); only where the mesh's own arrays have that form (fddh_problem_affine_info)
static int set_affine_geometry(fddh_problem &p, const char *, int value)
{
    for (auto &kv : p.domains) kv.second.set_affine_geometry(value != 0);
    if (p.subdomain) p.subdomain->set_affine_geometry(value != 0);
    operator_changed(p, {OperatorChange::arithmetic});
    return 0;
}

// the projection's passes as single launches of csrc/fdd_projection.hip (default where the kernel library has
// them) or composed from the multi-vector entries (projection.hpp); the basis stays
static int set_fused_projection(fddh_problem &p, const char *, int value)
{
    if (value != 0)
        if (const char *missing = fdd::missing_projection_entry()) return fail("fused_projection needs %s, which the loaded kernel library does not export", missing);
    p.fine().projection.fused = value != 0;
    return 0;
}

// a shift whose support is a small share of its vector (a Robin term alone) as a pass over the support
// (fdd_shift_add_indexed, boundary.hpp: kIndexedShiftShare) or, 0, as the dense pass; the same values either way
static int set_indexed_shift(fddh_problem &p, const char *, int value)
{
    if (value != 0)
        if (const char *missing = fdd::missing_indexed_shift_entry()) return fail("indexed_shift needs %s, which the loaded kernel library does not export", missing);
    for (auto &kv : p.domains) kv.second.indexed_shift = value != 0;
    if (p.subdomain) p.subdomain->indexed_shift = value != 0;
    return 0;
}

// the norm of the inner GMRES's last Arnoldi vector of a cycle from the projections (Subdomain::last_norm_from_projections)
// or, 0, from the exact pass as before: rounding differs, nothing else
static int set_last_norm_from_projections(fddh_problem &p, const char *, int value)
{
    if (value != 0)
        if (const char *missing = fdd::missing_norm_estimate_entry()) return fail("last_norm_from_projections needs %s, which the loaded kernel library does not export", missing);
    if (p.subdomain) p.subdomain->last_norm_from_projections = value != 0;
    return 0;
}

// 0: the inner FCG / GMRES(m) (set_options' preconditioner_type); 1: the Chebyshev-Jacobi iteration (an option of this
// build, Subdomain::chebyshev_dofs), which takes the place of either.  What it cannot run on is refused when a solve starts.
static int set_inner_solver(fddh_problem &p, const char *, int value)
{
    if (value != 0 && value != 1) return fail("inner_solver is 0 (FCG / GMRES) or 1 (Chebyshev-Jacobi)");
    p.subdomain->inner_solver = value;
    return 0;
}

static int set_inner_chebyshev_order(fddh_problem &p, const char *, int value)
{
    if (value < 1 || value > 16) return fail("inner_chebyshev_order must lie in 1..16, got %d", value);
    p.subdomain->cheby.order = value;
    return 0;
}

static int set_inner_chebyshev_lower_permille(fddh_problem &p, const char *, int value)
{
    if (value < 1 || value > 999) return fail("inner_chebyshev_lower_permille must lie in 1..999, got %d", value);
    if (!(value / 1000.0 < p.subdomain->cheby.upper)) return fail("inner_chebyshev_lower_permille %d is not below the upper factor %g", value, p.subdomain->cheby.upper);
    p.subdomain->cheby.lower = value / 1000.0;
    return 0;
}

// chebyshev_kernels: a step of the Chebyshev-Jacobi solve as one launch of fdd_cheby_step (default where the kernel
// library has it) or, 0, composed from vector_vector_addition / vector_diagonal_scaling_dev.  fused_chebyshev: the step
// as the epilogue of the gather in front of it where that applies (default likewise); 0: gather, then the step.
static int set_chebyshev_kernels(fddh_problem &p, const char *name, int value)
{
    const bool fused = strcmp(name, "fused_chebyshev") == 0;
    if (value != 0)
        if (const char *missing = fdd::missing_chebyshev_entry(fused)) return fail("%s needs %s, which the loaded kernel library does not export", name, missing);
    (fused ? p.subdomain->cheby.fused : p.subdomain->cheby.use_kernels) = value != 0;
    return 0;
}

static int set_amg_graph(fddh_problem &p, const char *, int value)
{
    if (p.subdomain) p.subdomain->amg_hierarchy.use_graph = value != 0;
    return 0;
}

static int set_amg_fused_smoother(fddh_problem &p, const char *, int value)
{
    if (p.subdomain) p.subdomain->amg_hierarchy.set_fused_smoother(value != 0);
    return 0;
}

// the interpolator of a geometric level applied from the lattice's weight table (fdd_lattice_prolong / _restrict)
// instead of as two SpMVs; 0: the CSR interpolator on every level (the same operator, sums in the CSR order)
static int set_amg_matrix_free_transfer(fddh_problem &p, const char *, int value)
{
    if (p.subdomain) p.subdomain->amg_hierarchy.set_matrix_free_transfer(value != 0);
    return 0;
}

// the reference's PTYPE = Float (config.hpp:19-20): 64 or 32 for the whole inner solve (Krylov vectors, element
// stiffness, gather, V-cycle)
static int set_preconditioner_precision(fddh_problem &p, const char *, int value)
{
    if (p.subdomain and not p.subdomain->set_precision(value)) return fail("preconditioner_precision is 64 or 32 (32: 3-D regions on the dof-space inner solve, Chebyshev order >= 2)");
    return 0;
}

// subdomain.hpp:236 `num_vcycles` (run.py:154 rewrites the line and rebuilds; here a run-time switch)
static int set_amg_num_vcycles(fddh_problem &p, const char *, int value)
{
    if (value < 1 || value > 16) return fail("amg_num_vcycles must lie in 1..16");
    p.subdomain->num_vcycles = value;
    p.subdomain->amg_hierarchy.set_num_vcycles(value);
    return 0;
}

// subdomain.hpp:237 `cheby_order` (run.py:155; clamped to 1..4 by subdomain.tpp:3477-3478).  The smoother's
// coefficients are computed when the hierarchy is built: set it before (fddh_problem_amg_build / first solve)
static int set_amg_cheby_order(fddh_problem &p, const char *, int value)
{
    if (value < 1 || value > 4) return fail("amg_cheby_order must lie in 1..4 (subdomain.tpp:3477-3478)");
    // -- or afterwards where the hierarchy is fddh_problem_amg_build's own: it is built again with the options of that
    // build.  One that was handed in level by level carries the caller's coefficients and cannot follow.
    Subdomain<PType> &sub = *p.subdomain;
    if (value == sub.cheby_order) return 0;
    if (value < 2 && (sub.amg_hierarchy.precision == 32 || sub.precision == 32)) return fail("amg_cheby_order %d: the 32-bit V-cycle (amg_precision / preconditioner_precision 32) needs a Chebyshev order of at least 2", value);
    if (sub.amg_hierarchy.ready() && !sub.amg_built_here) return fail("amg_cheby_order cannot change once a hierarchy has been handed in (fddh_problem_amg_add_level): its coefficients are the caller's");
    sub.cheby_order = value;
    if (sub.amg_hierarchy.ready()) sub.amg_rebuild();
    return 0;
}

// AMG/config.hpp:4 `Float`: 64 (double) or 32 (float)
static int set_amg_precision(fddh_problem &p, const char *, int value)
{
    if (p.subdomain and not p.subdomain->amg_hierarchy.set_precision(value)) return fail("amg_precision is 64 or 32 (32 needs a Chebyshev order of at least 2)");
    return 0;
}

// flag name -> the function that sets it, and whether a problem without a Subdomain refuses the flag (before the function runs)
struct CodedFlagRow
{
    const char *name;
    bool needs_subdomain;
    int (*set)(fddh_problem &p, const char *name, int value);
};

static const CodedFlagRow *coded_flag_row(const std::string &flag)
{
    static const CodedFlagRow table[] = {
        {"amg_device_setup", true, set_amg_device_setup},
        {"sub_use_preconditioner", true, set_sub_use_preconditioner},
        {"affine_geometry", false, set_affine_geometry},
        {"fused_projection", false, set_fused_projection},
        {"indexed_shift", false, set_indexed_shift},
        {"last_norm_from_projections", false, set_last_norm_from_projections},
        {"inner_solver", true, set_inner_solver},
        {"inner_chebyshev_order", true, set_inner_chebyshev_order},
        {"inner_chebyshev_lower_permille", true, set_inner_chebyshev_lower_permille},
        {"chebyshev_kernels", true, set_chebyshev_kernels},
        {"fused_chebyshev", true, set_chebyshev_kernels},
        {"amg_graph", false, set_amg_graph},
        {"amg_fused_smoother", false, set_amg_fused_smoother},
        {"amg_matrix_free_transfer", false, set_amg_matrix_free_transfer},
        {"preconditioner_precision", false, set_preconditioner_precision},
        {"amg_num_vcycles", true, set_amg_num_vcycles},
        {"amg_cheby_order", true, set_amg_cheby_order},
        {"amg_precision", false, set_amg_precision},
    };
    for (const CodedFlagRow &row : table)
        if (flag == row.name) return &row;
    return nullptr;
}

int fddh_problem_set_flag(fddh_problem *p, const char *name, int value)
{
    return on_problem(p, name != nullptr, [&](fddh_problem &pr) {
        const std::string s(name);
        if (const PlainFlagRow *row = plain_flag_row(s))
        {
            if (row->domain)
                for (auto &kv : pr.domains) kv.second.*row->domain = value != 0;
            if (row->subdomain && pr.subdomain) (*pr.subdomain).*row->subdomain = value != 0;
        }
        else if (fdd::stiffness_flag_row(s))
        {
            // the flags that choose between the stiffness kernels: what each does, the entries it needs and why none of them
            // empties what hangs on the operator are in element_operator.hpp (StiffnessFlags).  Refused before anything is written
            for (auto &kv : pr.domains) fdd::set_stiffness_flag(kv.second.stiffness, s, value != 0);
            if (pr.subdomain) fdd::set_stiffness_flag(pr.subdomain->stiffness, s, value != 0);
        }
        else if (const CodedFlagRow *coded = coded_flag_row(s))
        {
            if (coded->needs_subdomain && !pr.subdomain) return fail("problem was created without a Subdomain");
            return coded->set(pr, name, value);
        }
        else
            return fail("unknown flag '%s'", name);
        return 0;
    });
}

int fddh_problem_sub_point_dofs(const fddh_problem *p, int *dof, int n)
{
    return on_subdomain(p, dof != nullptr, [&](const fddh_problem &, const Subdomain<PType> &s) {
        if (n != (int)s.point_dof.size()) return fail("the subdomain region has %d points", (int)s.point_dof.size());
        memcpy(dof, s.point_dof.data(), (size_t)n * sizeof(int));
        return 0;
    });
}

int fddh_problem_amg_add_level(fddh_problem *p, int n, const int *A_ptr, const int *A_col, const double *A_val, const double *D_val, const double *coefs, int num_coefs, int n_coarse, const int *P_ptr, const int *P_col, const double *P_val)
{
    return on_subdomain(p, A_ptr && A_col && A_val && D_val && coefs, [&](fddh_problem &, Subdomain<PType> &s) {
        if (s.amg_hierarchy.ready()) return fail("the AMG hierarchy is already finalized");
        if (num_coefs != s.cheby_order) return fail("cheby_order is %d, got %d coefficients", s.cheby_order, num_coefs);
        if (s.amg_hierarchy.levels.empty() && n != s.dofs()) return fail("the finest AMG level must have the subdomain's %d dofs, got %d", s.dofs(), n);
        if (!s.amg_hierarchy.levels.empty())
        {
            const amg::Level &prev = s.amg_hierarchy.levels.back();
            if (prev.P.num_rows == 0) return fail("the previous level was given without a prolongation, so it is the coarsest");
            if (prev.P.num_cols != n) return fail("level size %d does not match the previous prolongation's %d columns", n, prev.P.num_cols);
        }
        if ((P_ptr != nullptr) != (n_coarse > 0)) return fail("n_coarse > 0 exactly when a prolongation is given");
        s.amg_add_level(n, A_ptr, A_col, A_val, D_val, coefs, n_coarse, P_ptr, P_col, P_val);
        return 0;
    });
}

int fddh_problem_amg_finalize(fddh_problem *p)
{
    return on_subdomain(p, true, [&](fddh_problem &, Subdomain<PType> &s) {
        if (s.amg_hierarchy.levels.empty()) return fail("no AMG level was added");
        if (s.amg_hierarchy.levels.back().P.num_rows != 0) return fail("the last AMG level still has a prolongation: add its coarse level first");
        s.amg_finalize();
        return 0;
    });
}

int fddh_problem_amg_build(fddh_problem *p, int coarsest_size, double strength, int smooth_prolongator, int verbose, int *num_levels)
{
    return on_subdomain(p, true, [&](fddh_problem &, Subdomain<PType> &s) {
        fdd::low_order::Options o;
        if (coarsest_size > 0) o.coarsest_size = coarsest_size;
        if (strength > 0.0) o.strength = strength;
        o.smooth_prolongator = smooth_prolongator != 0;
        const int nl = s.amg_build(o, verbose != 0);
        if (num_levels) *num_levels = nl;
        return 0;
    });
}

int fddh_problem_amg_level_info(const fddh_problem *p, int level, int *n, int *nnz_A, int *n_coarse, int *nnz_P)
{
    return on_problem(p, true, "no Subdomain", [&](const fddh_problem &pr) {
        if (!pr.subdomain) return fail("no Subdomain");
        const auto &lv = pr.subdomain->amg_hierarchy.levels;
        if (level < 0 || level >= (int)lv.size()) return fail("the hierarchy has %d levels", (int)lv.size());
        if (n) *n = lv[level].n;
        if (nnz_A) *nnz_A = lv[level].A.num_nnz;
        if (n_coarse) *n_coarse = lv[level].P.num_cols;
        if (nnz_P) *nnz_P = lv[level].P.num_nnz;
        return 0;
    });
}

int fddh_problem_amg_setup_info(const fddh_problem *p, int *levels_built_on_device, double *setup_seconds)
{
    return on_subdomain(p, true, [&](const fddh_problem &, const Subdomain<PType> &s) {
        if (levels_built_on_device) *levels_built_on_device = s.amg_levels_on_device;
        if (setup_seconds) *setup_seconds = s.amg_setup_seconds;
        return 0;
    });
}

int fddh_problem_amg_level_transfer(const fddh_problem *p, int level, int *matrix_free)
{
    return on_problem(p, true, "no Subdomain", [&](const fddh_problem &pr) {
        if (!pr.subdomain || !matrix_free) return fail("no Subdomain");
        const auto &H = pr.subdomain->amg_hierarchy;
        if (level < 0 || level >= (int)H.levels.size()) return fail("the hierarchy has %d levels", (int)H.levels.size());
        *matrix_free = (H.levels[level].T.active && H.matrix_free_transfer) ? 1 : 0;
        return 0;
    });
}

int fddh_problem_amg_level_arrays(const fddh_problem *p, int level, int *A_ptr, int *A_col, double *A_val, double *D_val, double *coefs, int *P_ptr, int *P_col, double *P_val)
{
    return on_problem(p, true, "no Subdomain", [&](const fddh_problem &pr) {
        if (!pr.subdomain) return fail("no Subdomain");
        auto &lv = pr.subdomain->amg_hierarchy.levels;
        if (level < 0 || level >= (int)lv.size()) return fail("the hierarchy has %d levels", (int)lv.size());
        amg::Level &L = lv[level];
        // col / val of a level built in HBM have no host copy: read from the device arrays
        auto fetch = [](CSR_Matrix<double> &M, int *col, double *val) {
            if (M.host_mirrors())
            {
                if (col) memcpy(col, M.col_hst.data(), M.col_hst.size() * sizeof(int));
                if (val) memcpy(val, M.val_hst.data(), M.val_hst.size() * sizeof(double));
            }
            else if (M.num_nnz > 0)
            {
                if (col) M.col.copyTo(col, (size_t)M.num_nnz * sizeof(int));
                if (val) M.val.copyTo(val, (size_t)M.num_nnz * sizeof(double));
            }
        };
        if (A_ptr) memcpy(A_ptr, L.A.ptr_hst.data(), L.A.ptr_hst.size() * sizeof(int));
        fetch(L.A, A_col, A_val);
        if (D_val) L.D_val.copyTo(D_val, (size_t)L.n * sizeof(double));
        if (coefs) memcpy(coefs, L.coefs.data(), L.coefs.size() * sizeof(double));
        if (L.P.num_rows > 0)
        {
            if (P_ptr) memcpy(P_ptr, L.P.ptr_hst.data(), L.P.ptr_hst.size() * sizeof(int));
            fetch(L.P, P_col, P_val);
        }
        return 0;
    });
}

// z = low_order_preconditioner(r) on level-0 subdomain points (subdomain.tpp:3987-4159)
int fddh_problem_amg_apply(fddh_problem *p, const double *r, double *z)
{
    return on_subdomain(p, r && z, [&](fddh_problem &pr, Subdomain<PType> &s) {
        if (!s.amg_hierarchy.ready()) return fail("no finalized AMG hierarchy is attached");
        fine_round_trip(pr, r, z, [&] { s.apply_low_order_preconditioner(pr.b, pr.a); });
        return 0;
    });
}

int fddh_problem_dssum(fddh_problem *p, double *out, const double *in, int apply_mask, int apply_weight)
{
    return on_problem(p, out && in, [&](fddh_problem &pr) {
        fine_round_trip(pr, in, out, [&] { pr.fine().direct_stiffness_summation(pr.b, pr.a, apply_mask != 0, apply_weight != 0); });
        return 0;
    });
}

int fddh_problem_stiffness(fddh_problem *p, double *out, const double *in, int apply_dssum)
{
    return on_problem(p, out && in, [&](fddh_problem &pr) {
        fine_round_trip(pr, in, out, [&] { pr.fine().stiffness_matrix(pr.b, pr.a, apply_dssum != 0); });
        return 0;
    });
}

// ---- fddh_field_*: mass, gradient and weak divergence on the fine level (field_ops.hpp) ----
int fddh_field_mass(fddh_problem *p, double *mass)
{
    return on_field_ops(p, mass != nullptr, [&](fddh_problem &pr, const fdd::FieldOps<Domain<SType>> &ops) {
        ops.mass(pr.b);
        pr.b.copyTo(mass, fine_bytes(pr));
        return 0;
    });
}

int fddh_field_gradient(fddh_problem *p, const double *u, double *gx, double *gy, double *gz, int average)
{
    return on_field_ops(p, u && gx && gy && gz, [&](fddh_problem &pr, const fdd::FieldOps<Domain<SType>> &ops) {
        fdd::memory third = fdd::dev().malloc<double>(pr.fine().num_local_points);
        pr.a.copyFrom(u, fine_bytes(pr));
        ops.gradient(pr.b, pr.c, third, pr.a);
        fdd::memory *g[3] = {&pr.b, &pr.c, &third};
        double *out[3] = {gx, gy, gz};
        for (int a = 0; a < 3; a++)
        {
            if (average) // the multiplicity-weighted mean over the copies of a node: continuous; collective on several ranks
            {
                pr.fine().direct_stiffness_summation(pr.a, *g[a], false, true);
                pr.a.copyTo(out[a], fine_bytes(pr));
            }
            else
                g[a]->copyTo(out[a], fine_bytes(pr));
        }
        return 0;
    });
}

int fddh_field_weak_divergence(fddh_problem *p, const double *vx, const double *vy, const double *vz, double *out)
{
    return on_field_ops(p, vx && vy && vz && out, [&](fddh_problem &pr, const fdd::FieldOps<Domain<SType>> &ops) {
        fdd::memory result = fdd::dev().malloc<double>(pr.fine().num_local_points);
        pr.a.copyFrom(vx, fine_bytes(pr));
        pr.b.copyFrom(vy, fine_bytes(pr));
        pr.c.copyFrom(vz, fine_bytes(pr));
        ops.weak_divergence(result, pr.a, pr.b, pr.c);
        result.copyTo(out, fine_bytes(pr));
        return 0;
    });
}

// ---- the convection term c . grad u on the fine level: pointwise, and as the over-integrated weak form (field_ops.hpp) ----
int fddh_convect(fddh_problem *p, const double *cx, const double *cy, const double *cz, const double *u, double *out)
{
    return convect_entry(p, cx, cy, cz, u, out, [](const fdd::FieldOps<Domain<SType>> &ops, fdd::memory &result, auto &...in) { ops.convect(result, in...); });
}

int fddh_weak_convect(fddh_problem *p, const double *cx, const double *cy, const double *cz, const double *u, double *out)
{
    return convect_entry(p, cx, cy, cz, u, out, [](const fdd::FieldOps<Domain<SType>> &ops, fdd::memory &result, auto &...in) { ops.weak_convect(result, in...); });
}

// the host tables of the weak form's quadrature; no kernel is needed
int fddh_convect_quadrature(fddh_problem *p, int *num_quad, double *z, double *w, double *P, double *Pd)
{
    return on_problem(p, true, [&](fddh_problem &pr) {
        Domain<SType> &d = pr.fine();
        if (d.poly_degree < 1) return fail("the quadrature of the convection term needs poly_degree >= 1, got %d", d.poly_degree);
        fdd::FieldGeometry &g = d.field_geometry;
        g.quadrature(d.D_hat_hst, d.poly_degree);
        if (num_quad) *num_quad = g.num_quad;
        if (z) memcpy(z, g.quad_z.data(), g.quad_z.size() * sizeof(double));
        if (w) memcpy(w, g.quad_w.data(), g.quad_w.size() * sizeof(double));
        if (P) memcpy(P, g.P_hst.data(), g.P_hst.size() * sizeof(double));
        if (Pd) memcpy(Pd, g.Pd_hst.data(), g.Pd_hst.size() * sizeof(double));
        return 0;
    });
}

int fddh_inner_norm_counters(fddh_problem *p, long long *estimated, long long *exact, double *min_ratio)
{
    return on_subdomain(p, true, [&](fddh_problem &, Subdomain<PType> &s) {
        long long e = 0, x = 0;
        double r = 0.0;
        s.norm_counters(e, x, r);
        if (estimated) *estimated = e;
        if (exact) *exact = x;
        if (min_ratio) *min_ratio = r;
        return 0;
    });
}

// The zeroth-order term of the operator from the two terms a caller sets, for both setters (fddh_helmholtz_set,
// fddh_boundary_robin_set): per point the product lambda_q B_q where a lambda is set, otherwise 0.0, then + r[q] where a
// Robin coefficient is set; Domain::set_shift sums the points into nodes, the Subdomain takes the node vector in its dofs, and
// what hangs on the operator is emptied.  With no Robin coefficient the statements are those of a Helmholtz shift alone.
static void rebuild_shift(fddh_problem &pr)
{
    Domain<SType> &d = pr.fine();
    const size_t np = (size_t)d.num_local_points;
    const bool was_active = d.shift_active();
    if (pr.robin_r.empty())
        d.set_shift(pr.lambda_B.empty() ? nullptr : pr.lambda_B.data());
    else
    {
        std::vector<double> c = pr.lambda_B.empty() ? std::vector<double>(np, 0.0) : pr.lambda_B;
        for (size_t q = 0; q < np; q++) c[q] = c[q] + pr.robin_r[q];
        d.set_shift(c.data());
    }
    if (Subdomain<PType> *s = pr.subdomain.get())
        s->set_shift(d.shift_active() ? fdd::helmholtz::dofs_of_nodes(d.shift_nodes_hst, d.scatter_matrix().col_hst.data(), s->point_dof.data(), np, s->dof_count()) : std::vector<double>());
    operator_changed(pr, OperatorChange::of_shift(was_active));
}

// ---- fddh_helmholtz_*: -laplace(u) + lambda u through the node-space outer solve and the dof-space inner solve ----
int fddh_helmholtz_set(fddh_problem *p, double lambda, const double *lambda_points)
{
    return on_problem(p, true, [&](fddh_problem &pr) {
        Domain<SType> &d = pr.fine();
        const size_t np = (size_t)d.num_local_points;
        const std::string why = fdd::helmholtz::refusal(fdd::missing_helmholtz_entry(), fdd::comm().size, d.mesh.dim, d.poly_degree, pr.subdomain && pr.subdomain->composite(), pr.subdomain ? (long long)pr.subdomain->point_dof.size() : -1, lambda, lambda_points, (long long)np);
        if (!why.empty()) return fail("%s", why.c_str());
        const auto range = lambda_points && np ? std::minmax_element(lambda_points, lambda_points + np) : std::make_pair(&lambda, &lambda);
        const double lo = *range.first, hi = *range.second;
        std::vector<double> lambda_B;
        if (hi > 0.0)
        {
            fdd::FieldOps<Domain<SType>>(d).mass(pr.b);
            lambda_B.resize(np);
            pr.b.copyTo(lambda_B.data(), fine_bytes(pr));
            fdd::helmholtz::scale_mass(lambda_B, lambda, lambda_points);
        }
        pr.lambda_B = std::move(lambda_B);
        pr.helmholtz_min = hi > 0.0 ? lo : 0.0;
        pr.helmholtz_max = hi > 0.0 ? hi : 0.0;
        rebuild_shift(pr);
        return 0;
    });
}

int fddh_helmholtz_info(fddh_problem *p, int *active, double *min, double *max)
{
    return on_problem(p, true, [&](fddh_problem &pr) {
        if (active) *active = pr.lambda_B.empty() ? 0 : 1;
        if (min) *min = pr.helmholtz_min;
        if (max) *max = pr.helmholtz_max;
        return 0;
    });
}

int fddh_helmholtz_shift(fddh_problem *p, double *cbar_nodes, int n)
{
    return on_problem(p, cbar_nodes != nullptr, [&](fddh_problem &pr) {
        const Domain<SType> &d = pr.fine();
        if (n != d.num_local_nodes) return fail("the shift has %d entries (the rank's nodes), got %d", d.num_local_nodes, n);
        for (int i = 0; i < n; i++) cbar_nodes[i] = d.shift_active() ? d.shift_nodes_hst[i] : 0.0;
        return 0;
    });
}

int fddh_helmholtz_node_operator(fddh_problem *p, const double *v_nodes, double *q_nodes, int n, double *vq)
{
    return on_problem(p, v_nodes && q_nodes, [&](fddh_problem &pr) {
        Domain<SType> &d = pr.fine();
        if (d.mesh.dim != 3 || d.poly_degree > 15 || !d.gather_matrix().unit_values) return fail("the node-space operator needs a 3-D problem of degree 1..15 with a boolean gather");
        if (n != d.num_local_nodes) return fail("node vectors have %d entries, got %d", d.num_local_nodes, n);
        fdd::memory vn = fdd::dev().malloc<double>(std::max(n, 1)), qn = fdd::dev().malloc<double>(std::max(n, 1));
        vn.copyFrom(v_nodes, (size_t)n * sizeof(double));
        const double dot = d.node_operator(qn, vn);
        qn.copyTo(q_nodes, (size_t)n * sizeof(double));
        if (vq) *vq = dot;
        return 0;
    });
}

// ---- fddh_boundary_*: Neumann and Robin faces of the generated meshes (host/boundary.hpp) ----
// why the face entries cannot run on this problem, or nullptr
static const char *face_list_refusal(const fddh_problem &pr)
{
    if (!pr.generated) return "this problem was made from mesh files and has no face list: the boundary entries know the faces of the generated box meshes only";
    if (pr.fine().mesh.dim != 3) return "the boundary entries are 3-D only";
    return nullptr;
}

// area (and, where normal[0] is given, the three components of the normal) of every point of the problem's face list, on the host
static int face_surface(fddh_problem &pr, double *area, double *const normal[3])
{
    Domain<SType> &d = pr.fine();
    if (const char *missing = fdd::missing_boundary_entry()) return fail("the surface weights need %s, which the loaded kernel library does not export", missing);
    if (d.poly_degree < 1 || d.poly_degree > 15) return fail("the surface weights support poly_degree 1..15, got %d", d.poly_degree);
    const int m = pr.faces.size(), n = d.poly_degree + 1;
    if (m == 0) return 0;
    const size_t count = (size_t)m * n * n;
    if (pr.face_elem_dev.size() == 0)
    {
        pr.face_elem_dev = fdd::dev().malloc<int>(m);
        pr.face_elem_dev.copyFrom(pr.faces.elem.data(), m * sizeof(int));
        pr.face_side_dev = fdd::dev().malloc<int>(m);
        pr.face_side_dev.copyFrom(pr.faces.side.data(), m * sizeof(int));
    }
    d.field_geometry.upload(d.mesh, d.poly_degree);
    const double *X[3];
    for (int a = 0; a < 3; a++) X[a] = d.field_geometry.xyz[a].as<double>();
    fdd::memory out[4];
    const int num_out = normal ? 4 : 1;
    for (int o = 0; o < num_out; o++) out[o] = fdd::dev().malloc<double>(count);
    double *const nrm[3] = {out[1].as<double>(), out[2].as<double>(), out[3].as<double>()};
    FDD_CALL(fdd_field_surface(out[0].as<double>(), normal ? nrm : nullptr, X, d.D_hat.as<double>(), d.field_geometry.weights.as<double>(), pr.face_elem_dev.as<int>(), pr.face_side_dev.as<int>(), m, d.num_local_elements,
                               d.poly_degree, fdd::dev().stream));
    out[0].copyTo(area, count * sizeof(double));
    for (int a = 0; normal && a < 3; a++) out[1 + a].copyTo(normal[a], count * sizeof(double));
    return 0;
}

int fddh_boundary_info(fddh_problem *p, char *faces_out, int *num_faces, int *robin_active, double *alpha_min, double *alpha_max, long long *shift_support, int *indexed_shift, int *indexed_in_use)
{
    return on_problem(p, true, [&](fddh_problem &pr) {
        Domain<SType> &d = pr.fine();
        if (faces_out)
        {
            memcpy(faces_out, pr.generated ? pr.spec.faces : "\0\0\0\0\0\0", 6);
            faces_out[6] = '\0';
        }
        if (num_faces) *num_faces = pr.generated ? pr.faces.size() : -1;
        if (robin_active) *robin_active = pr.robin_r.empty() ? 0 : 1;
        if (alpha_min) *alpha_min = pr.robin_min;
        if (alpha_max) *alpha_max = pr.robin_max;
        if (shift_support) *shift_support = d.shift_active() ? d.shift_support.count : 0;
        if (indexed_shift) *indexed_shift = d.indexed_shift ? 1 : 0;
        if (indexed_in_use) *indexed_in_use = (d.shift_indexed() ? 1 : 0) | (pr.subdomain && pr.subdomain->shift_indexed() ? 2 : 0);
        return 0;
    });
}

int fddh_boundary_faces(fddh_problem *p, int *elem, int *side, int m)
{
    return on_problem(p, elem && side, [&](fddh_problem &pr) {
        if (const char *why = face_list_refusal(pr)) return fail("%s", why);
        if (m != pr.faces.size()) return fail("the face list has %d entries, got %d", pr.faces.size(), m);
        for (int f = 0; f < m; f++)
        {
            elem[f] = pr.faces.elem[f];
            side[f] = pr.faces.side[f];
        }
        return 0;
    });
}

int fddh_boundary_surface(fddh_problem *p, double *area, double *nx, double *ny, double *nz, long long count)
{
    return on_problem(p, area != nullptr && (bool(nx) == bool(ny)) && (bool(ny) == bool(nz)), [&](fddh_problem &pr) {
        if (const char *why = face_list_refusal(pr)) return fail("%s", why);
        const long long n = pr.poly_degree + 1, want = (long long)pr.faces.size() * n * n;
        if (count != want) return fail("the surface arrays have %lld entries (faces x (N+1)^2), got %lld", want, count);
        double *const normal[3] = {nx, ny, nz};
        return face_surface(pr, area, nx ? normal : nullptr);
    });
}

int fddh_boundary_robin_set(fddh_problem *p, const double *alpha_face_points)
{
    return on_problem(p, true, [&](fddh_problem &pr) {
        if (const char *why = face_list_refusal(pr)) return fail("%s", why);
        Domain<SType> &d = pr.fine();
        if (alpha_face_points == nullptr)
        {
            if (pr.robin_r.empty()) return 0;
            pr.robin_r.clear();
            pr.robin_min = pr.robin_max = 0.0;
            rebuild_shift(pr);
            return 0;
        }
        if (const char *missing = fdd::missing_boundary_entry()) return fail("a Robin coefficient needs %s, which the loaded kernel library does not export", missing);
        const size_t np = (size_t)d.num_local_points;
        std::string why = fdd::helmholtz::refusal(fdd::missing_helmholtz_entry(), fdd::comm().size, d.mesh.dim, d.poly_degree, pr.subdomain && pr.subdomain->composite(), pr.subdomain ? (long long)pr.subdomain->point_dof.size() : -1, 0.0, nullptr, (long long)np);
        const int n = d.poly_degree + 1;
        if (why.empty()) why = fdd::boundary::robin_refusal(alpha_face_points, pr.faces, n, d.mesh.p_mask);
        if (!why.empty()) return fail("%s", why.c_str());
        const size_t count = (size_t)pr.faces.size() * n * n;
        const auto range = count ? std::minmax_element(alpha_face_points, alpha_face_points + count) : std::make_pair(alpha_face_points, alpha_face_points);
        const double lo = count ? *range.first : 0.0, hi = count ? *range.second : 0.0;
        std::vector<double> r;
        if (hi > 0.0)
        {
            std::vector<double> area(count);
            if (int rc = face_surface(pr, area.data(), nullptr)) return rc;
            r = fdd::boundary::robin_points(alpha_face_points, area.data(), pr.faces, n, np);
        }
        if (r.empty() && pr.robin_r.empty()) return 0; // an all-zero alpha on a problem without one: nothing changes
        pr.robin_r = std::move(r);
        pr.robin_min = hi > 0.0 ? lo : 0.0;
        pr.robin_max = hi > 0.0 ? hi : 0.0;
        rebuild_shift(pr);
        return 0;
    });
}

// ---- fddh_diffusivity_*: -div(kappa grad u), kappa per point of the fine level (host/diffusivity.hpp) ----
int fddh_diffusivity_set(fddh_problem *p, const double *kappa_points, int n)
{
    return on_problem(p, true, [&](fddh_problem &pr) {
        Domain<SType> &d = pr.fine();
        const std::string why = fdd::diffusivity::refusal(kappa_points, n, d.num_local_points, d.mesh.dim, fdd::comm().size, pr.subdomain && pr.subdomain->composite());
        if (!why.empty()) return fail("%s", why.c_str());
        if (pr.subdomain && (int)pr.subdomain->point_dof.size() != d.num_local_points) return fail("a diffusivity needs a Subdomain over the rank's own points");
        if (kappa_points == nullptr && !d.diffusivity_active()) return 0;
        d.set_diffusivity(kappa_points);
        if (pr.subdomain) pr.subdomain->set_diffusivity(kappa_points, (size_t)d.num_local_points, d.operator_list());
        operator_changed(pr, {OperatorChange::factors}); // solve_projected stays allowed: the images stored from here on are this operator's
        pr.diffusivity_min = kappa_points ? *std::min_element(kappa_points, kappa_points + n) : 0.0;
        pr.diffusivity_max = kappa_points ? *std::max_element(kappa_points, kappa_points + n) : 0.0;
        return 0;
    });
}

int fddh_diffusivity_info(fddh_problem *p, int *active, double *min, double *max, int *fine_domain_in_kernel, int *sub_lists_in_kernel, int *sub_lists)
{
    int enabled = 0;
    if (int rc = stiffness_info(p, "coefficient_in_kernel", &fdd::StiffnessChoice::coef_lines, &enabled, fine_domain_in_kernel, sub_lists_in_kernel, sub_lists)) return rc;
    return on_problem(p, true, [&](fddh_problem &pr) {
        if (active) *active = pr.fine().diffusivity_active() ? 1 : 0;
        if (min) *min = pr.diffusivity_min;
        if (max) *max = pr.diffusivity_max;
        return 0;
    });
}

int fddh_problem_residual_norm(fddh_problem *p, const double *r, double *norm)
{
    return on_problem(p, r && norm, [&](fddh_problem &pr) {
        Domain<SType> &d = pr.fine();
        // ||r|| = sqrt(<r, r>) through the public pieces (Domain::residual_norm is private, domain.hpp:71)
        pr.a.copyFrom(r, fine_bytes(pr));
        d.direct_stiffness_summation(pr.b, pr.a);
        fdd::memory ws = fdd::dev().malloc<double>(fdd_reduce_workspace_doubles());
        fdd::memory sc = fdd::dev().malloc<double>(1);
        FDD_CALL(fdd_dom_residual_norm(sc.as<double>(), ws.as<double>(), pr.a.as<double>(), pr.b.as<double>(), d.dirichlet_mask_memory().as<double>(), d.num_local_points, fdd::dev().stream));
        if (fdd::comm().size > 1) fdd::comm().allreduce_sum(sc.as<double>(), 1);
        double v = 0.0;
        sc.copyTo(&v, sizeof(double));
        *norm = std::sqrt(v);
        return 0;
    });
}

int fddh_problem_make_rhs(fddh_problem *p, int function_id, unsigned long long seed, double *u_star, double *f)
{
    return on_problem(p, true, [&](fddh_problem &pr) {
        Domain<SType> &d = pr.fine();
        d.initial_function(pr.a, function_id, seed); // poisson.cpp:211-213
        d.stiffness_matrix(pr.b, pr.a);              // poisson.cpp:219 (no dssum)
        if (u_star) pr.a.copyTo(u_star, fine_bytes(pr));
        if (f) pr.b.copyTo(f, fine_bytes(pr));
        return 0;
    });
}

int fddh_problem_make_rhs_from(fddh_problem *p, double *u_star_inout, double *f)
{
    return on_problem(p, u_star_inout != nullptr, [&](fddh_problem &pr) {
        Domain<SType> &d = pr.fine();
        pr.a.copyFrom(u_star_inout, fine_bytes(pr));
        d.direct_stiffness_summation(pr.a, pr.a, true, true); // domain.tpp:579
        d.stiffness_matrix(pr.b, pr.a);
        pr.a.copyTo(u_star_inout, fine_bytes(pr));
        if (f) pr.b.copyTo(f, fine_bytes(pr));
        return 0;
    });
}

int fddh_problem_solve(fddh_problem *p, int solver_id, const double *f, double *u, double *history, int history_cap, int *num_history, int *num_iterations)
{
    return on_problem(p, f && u, [&](fddh_problem &pr) {
        if (const char *why = helmholtz_outer_refusal(pr, solver_id != 0)) return fail("%s", why);
        return outer_solve(pr, f, u, history, history_cap, num_history, num_iterations, nullptr, [&](Domain<SType> &d, auto &preconditioner) { krylov_solve(pr, d, preconditioner, solver_id); });
    });
}

int fddh_problem_solve_timed(fddh_problem *p, int solver_id, const double *f, double *u, double *history, int history_cap, int *num_history, int *num_iterations, double *seconds)
{
    return on_problem(p, f && seconds, [&](fddh_problem &pr) {
        if (const char *why = helmholtz_outer_refusal(pr, solver_id != 0)) return fail("%s", why);
        return outer_solve(pr, f, u, history, history_cap, num_history, num_iterations, seconds, [&](Domain<SType> &d, auto &preconditioner) { krylov_solve(pr, d, preconditioner, solver_id); });
    });
}

int fddh_problem_projection_configure(fddh_problem *p, int capacity)
{
    return on_problem(p, true, [&](fddh_problem &pr) {
        if (capacity < 0 || capacity > FDD_PROJECTION_MAX) return fail("capacity %d: the projection basis holds 0 (off) to %d vectors", capacity, FDD_PROJECTION_MAX);
        Domain<SType> &d = pr.fine();
        d.projection.configure(capacity, d.num_local_points);
        return 0;
    });
}

int fddh_problem_projection_clear(fddh_problem *p)
{
    return on_problem(p, true, [&](fddh_problem &pr) {
        pr.fine().projection.clear();
        return 0;
    });
}

int fddh_problem_projection_info(const fddh_problem *p, int *capacity, int *size, long long *restarts)
{
    return on_problem(p, true, [&](const fddh_problem &pr) {
        const fdd::Projection &pj = pr.fine().projection;
        if (capacity) *capacity = pj.capacity;
        if (size) *size = pj.size;
        if (restarts) *restarts = pj.restarts;
        return 0;
    });
}

int fddh_problem_projection_basis(const fddh_problem *p, int k, double *x, double *Ax)
{
    return on_problem(p, true, [&](const fddh_problem &pr) {
        const fdd::Projection &pj = pr.fine().projection;
        if (k < 0 || k >= pj.size) return fail("k = %d: the projection basis holds %d vectors", k, pj.size);
        const size_t bytes = (size_t)pj.n * sizeof(double);
        if (x && bytes) pj.X.slice((size_t)k * pj.ld, pj.n).copyTo(x, bytes);
        if (Ax && bytes) pj.AX.slice((size_t)k * pj.ld, pj.n).copyTo(Ax, bytes);
        return 0;
    });
}

int fddh_problem_solve_projected(fddh_problem *p, int solver_id, const double *f, double *u, double *history, int history_cap, int *num_history, int *num_iterations, double *projection, double *seconds)
{
    return on_problem(p, f && u, [&](fddh_problem &pr) {
        if (pr.fine().shift_active()) return fail("solve_projected while a Helmholtz shift is set: the basis and its stored images belong to the operator without the term (clear the shift, or use solve)");
        double proj[4];
        if (int rc = outer_solve(pr, f, u, history, history_cap, num_history, num_iterations, seconds, [&](Domain<SType> &d, auto &preconditioner) { d.solve_projected(pr.b, pr.a, preconditioner, solver_id, proj); })) return rc;
        if (projection) memcpy(projection, proj, sizeof(proj));
        return 0;
    });
}

int fddh_problem_precond_apply(fddh_problem *p, int type, const double *r, double *z, double *history, int history_cap, int *num_history)
{
    return on_subdomain(p, r && z, [&](fddh_problem &pr, Subdomain<PType> &s) {
        if (const char *why = inner_solver_refusal(pr)) return fail("%s", why);
        if (const char *why = helmholtz_inner_refusal(pr, type == 0)) return fail("%s", why);
        if (const char *why = singular_refusal(pr)) return fail("%s", why);
        fine_round_trip(pr, r, z, [&] {
            if (type == 0)
                s.flexible_conjugate_gradient(pr.b, pr.a);
            else
                s.generalized_minimum_residual(pr.b, pr.a);
        });
        s.finish_history();
        copy_history(s.residual_history, history, history_cap, num_history);
        return 0;
    });
}

int fddh_problem_sub_op(fddh_problem *p, int op, const double *in, double *out)
{
    return on_subdomain(p, in && out, [&](fddh_problem &pr, Subdomain<PType> &s) {
        if (op == 0)
        {
            // tree_operator: input is an outer (Domain) vector
            pr.a.copyFrom(in, fine_bytes(pr));
            s.apply_tree_operator(pr.sb, pr.a);
            pr.sb.copyTo(out, sub_bytes(pr));
        }
        else if (op == 1)
            sub_round_trip(pr, in, out, [&] { s.stiffness_matrix(pr.sb, pr.sa); });
        else if (op == 2)
            sub_round_trip(pr, in, out, [&] { s.direct_stiffness_summation(pr.sb, pr.sa); });
        else
            return fail("unknown subdomain op %d", op);
        return 0;
    });
}

int fddh_problem_sub_dof_op(fddh_problem *p, int op, const double *in, double *out, int n)
{
    return on_subdomain(p, in && out, [&](fddh_problem &pr, Subdomain<PType> &s) {
        if (not s.dof_space_available()) return fail("the inner iteration of this problem does not run in dof space");
        if (n != s.dof_count()) return fail("dof vectors have %d entries, got %d", s.dof_count(), n);
        if (op == 0)
            s.host_operator_dofs(out, in);
        else if (op == 1)
        {
            pr.a.copyFrom(in, fine_bytes(pr));
            s.host_rhs_dofs(out, pr.a);
        }
        else
            return fail("unknown dof-space op %d", op);
        return 0;
    });
}

int fddh_problem_sub_jacobi_diagonal(fddh_problem *p, double *out, int n)
{
    return on_subdomain(p, out != nullptr, [&](fddh_problem &, Subdomain<PType> &s) {
        const std::vector<double> &d = s.jacobi_diagonal();
        if (n != s.dofs()) return fail("the diagonal has %d entries, got %d", s.dofs(), n);
        for (int i = 0; i < n; i++) out[i] = d[i];
        return 0;
    });
}

int fddh_problem_sub_dof_solve(fddh_problem *p, const double *fa, double *ua, int n)
{
    return on_subdomain(p, fa && ua, [&](fddh_problem &pr, Subdomain<PType> &s) {
        if (const char *why = inner_solver_refusal(pr)) return fail("%s", why);
        if (const char *why = helmholtz_inner_refusal(pr)) return fail("%s", why);
        if (not s.dof_space_available()) return fail("the inner iteration of this problem does not run in dof space");
        if (n != s.dof_count()) return fail("dof vectors have %d entries, got %d", s.dof_count(), n);
        s.host_solve_dofs(ua, fa);
        return 0;
    });
}

int fddh_problem_inner_chebyshev_configure(fddh_problem *p, int order, double lower, double upper, int power_iterations)
{
    return on_subdomain(p, true, [&](fddh_problem &, Subdomain<PType> &s) {
        if (order < 1 || order > 16) return fail("the Chebyshev order must lie in 1..16, got %d", order);
        if (!(lower > 0.0) || !(upper > lower) || !std::isfinite(upper)) return fail("the Chebyshev interval needs 0 < lower < upper, got [%g, %g]", lower, upper);
        if (power_iterations < 1 || power_iterations > 10000) return fail("power_iterations must lie in 1..10000, got %d", power_iterations);
        auto &c = s.cheby;
        c.order = order;
        c.lower = lower;
        c.upper = upper;
        if (power_iterations != c.power_iterations) c.lambda = 0.0; // the estimate belongs to its iteration count; the factors do not touch it
        c.power_iterations = power_iterations;
        return 0;
    });
}

int fddh_problem_inner_chebyshev_info(fddh_problem *p, int *order, double *lower, double *upper, double *lambda, int *power_iterations)
{
    return on_subdomain(p, true, [&](fddh_problem &, Subdomain<PType> &s) {
        if (lambda)
        {
            if (not s.dof_space_available()) return fail("the inner iteration of this problem does not run in dof space: there is no operator to bound");
            *lambda = s.chebyshev_lambda();
        }
        if (order) *order = s.cheby.order;
        if (lower) *lower = s.cheby.lower;
        if (upper) *upper = s.cheby.upper;
        if (power_iterations) *power_iterations = s.cheby.power_iterations;
        return 0;
    });
}

int fddh_problem_sub_residual_norm(fddh_problem *p, const double *r, double *norm)
{
    return on_subdomain(p, r && norm, [&](fddh_problem &pr, Subdomain<PType> &s) {
        pr.sa.copyFrom(r, sub_bytes(pr));
        s.compute_residual_norm(*norm, pr.sa);
        return 0;
    });
}

int fddh_problem_pcg_begin(fddh_problem *p, const double *f)
{
    return on_problem(p, f != nullptr, [&](fddh_problem &pr) {
        if (const char *why = outer_solve_refusal(pr)) return fail("%s", why);
        if (const char *why = helmholtz_outer_refusal(pr, false)) return fail("%s", why);
        if (const char *why = singular_refusal(pr)) return fail("%s", why);
        Domain<SType> &d = pr.fine();
        pr.a.copyFrom(f, fine_bytes(pr));
        with_preconditioner(pr, pr.subdomain && d.use_preconditioner, [&](auto &preconditioner) { d.fcg_begin(pr.b, pr.a, preconditioner); });
        return 0;
    });
}

int fddh_problem_pcg_steps(fddh_problem *p, int steps, double *last_residual)
{
    return on_problem(p, steps >= 0, "bad argument", [&](fddh_problem &pr) {
        if (const char *why = outer_solve_refusal(pr)) return fail("%s", why);
        if (const char *why = helmholtz_outer_refusal(pr, false)) return fail("%s", why);
        Domain<SType> &d = pr.fine();
        const double r = with_preconditioner(pr, pr.subdomain && d.use_preconditioner, [&](auto &preconditioner) { return d.fcg_steps(preconditioner, steps); });
        if (last_residual) *last_residual = r;
        return 0;
    });
}

int fddh_problem_pcg_solution(fddh_problem *p, double *u)
{
    return on_problem(p, u != nullptr, [&](fddh_problem &pr) {
        pr.fine().fcg_finish();
        pr.b.copyTo(u, fine_bytes(pr));
        return 0;
    });
}

// Average launch time of the assembly SpMVs on the problem's own matrices, timed with
// events on the stream (the "SpMV GB/s" half of the headline metric): which = 0: Q x
// (scatter, one non-zero per row), 1: Qt x (gather, 1-8 non-zeros per row).
int fddh_problem_spmv_time(fddh_problem *p, int which, int iterations, double *avg_us, double *algorithmic_bytes)
{
    return on_problem(p, avg_us && algorithmic_bytes && iterations >= 1 && which >= 0 && which <= 1, "bad argument", [&](fddh_problem &pr) {
        Domain<SType> &d = pr.fine();
        CSR_Matrix<SType> &A = (which == 0) ? d.scatter_matrix() : d.gather_matrix();
        fdd::memory x = fdd::dev().malloc<double>(std::max(A.num_cols, 1));
        fdd::memory y = fdd::dev().malloc<double>(std::max(A.num_rows, 1));
        FDD_CALL(fdd_set_to_value(x.as<double>(), 1.0, A.num_cols, 0, fdd::dev().stream));
        const float ms = spmv_ms(A, x, y, iterations);
        *avg_us = 1.0e3 * ms / iterations;
        *algorithmic_bytes = A.algorithmic_bytes(false);
        return 0;
    });
}

int fddh_problem_comm_time(fddh_problem *p, int iterations, double *avg_us, double *bytes)
{
    return on_problem(p, avg_us && bytes && iterations >= 1, "bad argument", [&](fddh_problem &pr) {
        for (int k = 0; k < FDDH_COMM_TIME_COUNT; k++) avg_us[k] = bytes[k] = 0.0;
        fdd::Comm &c = fdd::comm();
        if (c.size == 1) return 0;
        Domain<SType> &d = pr.fine();
        fdd::memory scal = fdd::dev().malloc<double>(4);
        FDD_CALL(fdd_memset(scal.ptr(), 0, 4 * sizeof(double), fdd::dev().stream));
        const auto clock = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        auto timed = [&](const std::function<void()> &op) {
            op(); // warm-up (first use of a peer pair may set up a connection)
            fdd::dev().finish();
            c.barrier();
            const double t0 = clock();
            for (int i = 0; i < iterations; i++) op();
            fdd::dev().finish();
            return 1.0e6 * (clock() - t0) / iterations;
        };
        // every rank makes the same calls in the same order
        avg_us[0] = timed([&] { c.allreduce_sum(scal.as<double>(), 3); });
        bytes[0] = 3 * sizeof(double);
        avg_us[1] = timed([&] { d.comm_probe_interface(2, false); });
        bytes[1] = 2.0 * d.interface_slots_count() * sizeof(double);
        avg_us[4] = timed([&] { d.comm_probe_interface(2, true); });
        bytes[4] = d.comm_interface_neighbour_bytes(2);
        if (pr.subdomain)
        {
            avg_us[2] = timed([&] { pr.subdomain->comm_probe_coarse(); });
            bytes[2] = pr.subdomain->comm_coarse_bytes();
            avg_us[3] = timed([&] { pr.subdomain->comm_probe_ring(); });
            bytes[3] = pr.subdomain->comm_ring_bytes();
            avg_us[5] = timed([&] { pr.subdomain->comm_probe_ring_and_coarse(); });
            bytes[5] = pr.subdomain->comm_ring_and_coarse_bytes();
        }
        return 0;
    });
}

int fddh_spmv_stencil_time(int m, int iterations, double *avg_us, double *algorithmic_bytes, long long *num_nnz)
{
    return guarded([&] {
        if (m < 2 || iterations < 1 || !avg_us || !algorithmic_bytes) return fail("bad argument");
        const long long n = (long long)m * m * m;
        if (n > 2000000000LL) return fail("grid too large");
        // rows in parallel ranges: counts first, then the entries (lexicographic neighbours = ascending columns)
        std::vector<int> ptr((size_t)n + 1, 0);
        auto span = [&](int i) { return (i == 0 || i == m - 1) ? 2 : 3; };
        for (int k = 0; k < m; k++)
            for (int j = 0; j < m; j++)
                for (int i = 0; i < m; i++) ptr[(size_t)i + (size_t)m * (j + (size_t)m * k) + 1] = span(i) * span(j) * span(k);
        long long total = 0;
        for (long long r = 0; r < n; r++)
        {
            total += ptr[r + 1];
            if (total > 2147483647LL) return fail("more than 2^31 non-zeros");
            ptr[r + 1] = (int)total;
        }
        std::vector<int> col((size_t)total);
        std::vector<double> val((size_t)total);
        fdd::low_order::parallel_ranges(n, fdd::low_order::range_parts(n), [&](long long r0, long long r1, int) {
            for (long long r = r0; r < r1; r++)
            {
                const int i = (int)(r % m), j = (int)((r / m) % m), k = (int)(r / ((long long)m * m));
                size_t at = (size_t)ptr[r];
                for (int dk = -1; dk <= 1; dk++)
                    for (int dj = -1; dj <= 1; dj++)
                        for (int di = -1; di <= 1; di++)
                        {
                            const int ii = i + di, jj = j + dj, kk = k + dk;
                            if (ii < 0 || jj < 0 || kk < 0 || ii >= m || jj >= m || kk >= m) continue;
                            const long long c = (long long)ii + (long long)m * (jj + (long long)m * kk);
                            col[at] = (int)c;
                            // trilinear stiffness stencil weights (8/3, 0, -1/6, -1/12 by neighbour class) times a seeded perturbation
                            const int cls = (di != 0) + (dj != 0) + (dk != 0);
                            const double base = (cls == 0) ? 8.0 / 3.0 : (cls == 1) ? -1.0e-3 : (cls == 2) ? -1.0 / 6.0 : -1.0 / 12.0;
                            val[at] = base * (1.0 + 1.0e-3 * (double)((r * 31 + c * 17) % 97));
                            at++;
                        }
            }
        });
        CSR_Matrix<SType> A;
        A.assemble_from_csr((int)n, (int)n, ptr.data(), col.data(), val.data());
        std::vector<int>().swap(col);
        std::vector<double>().swap(val);
        A.release_host();
        fdd::memory x = fdd::dev().malloc<double>((size_t)n);
        fdd::memory y = fdd::dev().malloc<double>((size_t)n);
        {
            std::vector<double> hx((size_t)n);
            for (long long r = 0; r < n; r++) hx[r] = 0.5 + 1.0e-3 * (double)((r * 7919) % 1009);
            x.copyFrom(hx.data(), (size_t)n * sizeof(double));
        }
        const float ms = spmv_ms(A, x, y, iterations);
        *avg_us = 1.0e3 * ms / iterations;
        *algorithmic_bytes = A.algorithmic_bytes(false);
        if (num_nnz) *num_nnz = total;
        return 0;
    });
}

int fddh_profile_enable(int on)
{
    return guarded([&] {
        fdd::profiler().reset();
        fdd::profiler().enabled = on != 0;
        fdd::profiler().only.clear();
        return 0;
    });
}

int fddh_profile_only(const char *kernel_key)
{
    return guarded([&] {
        fdd::profiler().only = kernel_key ? kernel_key : "";
        return 0;
    });
}

int fddh_profile_collect(char *json, size_t json_len)
{
    return guarded([&] {
        if (!json || json_len < 3) return fail("bad buffer");
        auto stats = fdd::profiler().collect();
        std::string s = "{";
        bool first = true;
        for (auto &kv : stats)
        {
            char item[512];
            snprintf(item, sizeof(item), "%s\"%s\": {\"count\": %lld, \"ms\": %.9g, \"bytes\": %.17g}", first ? "" : ", ", kv.first.c_str(), kv.second.count, kv.second.ms, kv.second.bytes);
            s += item;
            first = false;
        }
        s += "}";
        if (s.size() + 1 > json_len) return fail("profile JSON needs %zu bytes", s.size() + 1);
        memcpy(json, s.c_str(), s.size() + 1);
        return 0;
    });
}

int fddh_sync(void)
{
    return guarded([&] {
        fdd::dev().finish();
        return 0;
    });
}

int fddh_barrier(void)
{
    return guarded([&] {
        fdd::dev().finish();
        fdd::comm().barrier();
        fdd::dev().finish();
        return 0;
    });
}

} // extern "C"
