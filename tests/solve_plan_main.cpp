// Prints a solve's launch plan (csrc/solve_plan.inc, included alone) for the cases on the command line, eleven arguments
// each: program resto_ipopt B slots slots_resto split_it split_tr split_pair allow_pair ordered records.  Per case a
// "case" line, then a line per step:
//   KIND phase resto FORM team ckpt_it ckpt_tr
// With the single argument "ladder": for rows = 1 .. 200 a line "rows ksm_of(rows) K", K the compile-time size with_ksm
// hands its callable for mo4 = rows.
// Driven by tests/test_solve_plan_host.py, which builds it with the host compiler and its sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../mujoco-lip-mpc-simulation_amd/csrc/solve_plan.inc"

using namespace alip;

int main(int argc, char** argv)
{
    if (argc == 2 && std::strcmp(argv[1], "ladder") == 0) {
        for (int rows = 1; rows <= 200; ++rows) {
            int K = 0;
            with_ksm(rows, [&](auto k) { K = decltype(k)::value; });
            std::printf("%d %d %d\n", rows, ksm_of(rows), K);
        }
        return 0;
    }
    if (argc < 12 || (argc - 1) % 11 != 0) {
        std::fprintf(stderr,
                     "usage: %s ladder | (program resto_ipopt B slots slots_resto split_it split_tr split_pair allow_pair "
                     "ordered records)...\n",
                     argv[0]);
        return 2;
    }
    static const char* const programs[] = {"DD", "LANE", "WAVE_F64", "WAVE_F32", "SENS", "SENS_OBS"};
    static const char* const kinds[] = {"ZERO_HEADER", "ZERO_LIST", "DD", "LANE", "SENS", "SENS_OBS", "WAVE", "HANDOFF"};
    static const char* const forms[] = {"QUEUE", "ONE_WAVE", "TEAM", "PAIR"};
    for (int a = 1; a < argc; a += 11) {
        SpFacts f{};
        int prog = -1;
        for (int i = 0; i < 6; ++i)
            if (std::strcmp(argv[a], programs[i]) == 0) prog = i;
        if (prog < 0) {
            std::fprintf(stderr, "unknown program %s\n", argv[a]);
            return 2;
        }
        f.program = (SpProgram)prog;
        f.resto_ipopt = std::atoi(argv[a + 1]) != 0;
        f.B = std::atoll(argv[a + 2]);
        f.slots = std::atoll(argv[a + 3]);
        f.slots_resto = std::atoll(argv[a + 4]);
        f.split_it = std::atoi(argv[a + 5]);
        f.split_tr = std::atoi(argv[a + 6]);
        f.split_pair = std::atoi(argv[a + 7]) != 0;
        f.allow_pair = std::atoi(argv[a + 8]) != 0;
        f.ordered = std::atoi(argv[a + 9]) != 0;
        f.records = std::atoi(argv[a + 10]) != 0;
        std::printf("case %s\n", programs[prog]);
        for (const SpStep& s : solve_plan(f))
            std::printf("%s %d %d %s %d %d %d\n", kinds[s.kind], s.phase, (int)s.resto, forms[s.form], s.team, s.ckpt_it,
                        s.ckpt_tr);
    }
    return 0;
}
