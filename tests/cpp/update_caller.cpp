// tests/cpp/update_caller.cpp — a caller of the two osqp-eigen matrix updates, OsqpEigen::Solver::updateHessianMatrix
// and updateLinearConstraintsMatrix, against include/OsqpEigen/OsqpEigen.h and the caller's own Eigen (compiled with
// the flags of tests/cpp/Makefile's reference_caller).  Test program, not product code.
//
// Input (whitespace-separated numbers, from the test): n m, then P (n x n), A (m x n), q (n), l (m), u (m),
// P_new (n x n), A_new (m x n), row-major.  It sets the solver up on (P, q, A, l, u) and solves, hands it P_new
// and solves, hands it A_new and solves.
// Output: one line per solve, "status iterations x[0..n) y[0..m)" (%.17g).
// Exit: 0 ok; 3 initSolver() false (e.g. no gfx950 device); 4 a solve or an update returned false; 2 bad input.
#include <cstdio>
#include <fstream>

#include <OsqpEigen/OsqpEigen.h>

static bool read_sparse(std::istream &in, Eigen::SparseMatrix<double> &S, int rows, int cols)
{
    S.resize(rows, cols);
    for (int i = 0; i < rows; i++)
        for (int j = 0; j < cols; j++) {
            double v;
            if (!(in >> v)) return false;
            S.insert(i, j) = v;  // every entry, explicit zeros included, as the reference stores H and Gbar
        }
    S.makeCompressed();
    return true;
}

static bool read_vec(std::istream &in, Eigen::VectorXd &v, int len)
{
    v.resize(len);
    for (int i = 0; i < len; i++)
        if (!(in >> v(i))) return false;
    return true;
}

static bool solve_and_print(OsqpEigen::Solver &s)
{
    if (!s.solve()) {
        std::printf("solve failed: status %d (%s)\n", s.getStatus(), s.lastError().c_str());
        return false;
    }
    std::printf("%d %d", s.getStatus(), s.getIterations());
    for (int i = 0; i < s.getSolution().size(); i++) std::printf(" %.17g", s.getSolution()(i));
    for (int i = 0; i < s.getDualSolution().size(); i++) std::printf(" %.17g", s.getDualSolution()(i));
    std::printf("\n");
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    int n = 0, m = 0;
    Eigen::SparseMatrix<double> P, A, Pn, An;
    Eigen::VectorXd q, l, u;
    if (!(in >> n >> m) || n < 1 || m < 1 || !read_sparse(in, P, n, n) || !read_sparse(in, A, m, n) || !read_vec(in, q, n) ||
        !read_vec(in, l, m) || !read_vec(in, u, m) || !read_sparse(in, Pn, n, n) || !read_sparse(in, An, m, n))
        return 2;
    OsqpEigen::Solver solver;
    solver.settings()->setWarmStart(true);
    solver.data()->setNumberOfVariables(n);
    solver.data()->setNumberOfConstraints(m);
    if (!solver.data()->setHessianMatrix(P) || !solver.data()->setGradient(q) ||
        !solver.data()->setLinearConstraintsMatrix(A) || !solver.data()->setLowerBound(l) ||
        !solver.data()->setUpperBound(u) || !solver.initSolver()) {
        std::printf("initSolver failed: %s\n", solver.lastError().c_str());
        return 3;
    }
    if (!solve_and_print(solver)) return 4;
    if (!solver.updateHessianMatrix(Pn)) {
        std::printf("updateHessianMatrix failed: %s\n", solver.lastError().c_str());
        return 4;
    }
    if (!solve_and_print(solver)) return 4;
    if (!solver.updateLinearConstraintsMatrix(An)) {
        std::printf("updateLinearConstraintsMatrix failed: %s\n", solver.lastError().c_str());
        return 4;
    }
    if (!solve_and_print(solver)) return 4;
    return 0;
}
