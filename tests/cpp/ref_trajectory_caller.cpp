// tests/cpp/ref_trajectory_caller.cpp — a caller of the C++ ModelPredictiveControlAPI with a horizon reference
// (tests/test_ref_trajectory.py): two controllerSteps with a ramp reference set through
// updateRef(const std::vector<double> &), then one after updateRef(double) (the scalar path again); prints
// "U <value>" after each.  usage: ref_trajectory_caller CONFIG.json
#include <cstdio>
#include <vector>

#include "../../solvempc_amd/cpp/mpc_api.hpp"

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    ModelPredictiveControlAPI mpc(false, argv[1]);
    if (!mpc.solverFlag) return 1;
    const double x0[N_S] = {0.05, -0.02, 0.01, 0.1};
    for (int i = 0; i < N_S; i++) mpc.X(i) = x0[i];
    std::vector<double> ramp(mpc.horizon);
    for (int t = 0; t < mpc.horizon; t++) ramp[t] = 0.1 * t;
    mpc.updateRef(ramp);
    for (int k = 0; k < 2; k++) {
        if (!mpc.controllerStep()) return 3;
        std::printf("U %.17g\n", mpc.U(0));
    }
    mpc.updateRef(mpc.xref);
    if (!mpc.controllerStep()) return 4;
    std::printf("U %.17g\n", mpc.U(0));
    return 0;
}
