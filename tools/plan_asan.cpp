// plan_batch (csrc/gpsbb_plan.h) under the host sanitizers, on a machine without a GPU: the matrix of tests/test_batch_plan.py, as
// `python tests/batch_plan_cases.py FILE` writes it, through gpsbb_test_plan; prints what the test compares, one line per set-up —
// and, for every set-up with GPSBB_CHAIN_CARRIER and the IEEE carrier, what plan_push_side makes of it (gpsbb_test_push_side) and, on
// a line of its own ("chain ..."), what plan_chain_only makes of gpsbb_chain_carrier over the same blocks (gpsbb_test_chain_plan);
// and for every set-up, on a line of its own ("launch ..."), what plan_launch makes of one run of it (gpsbb_test_launch_plan) at 256
// and 8 CUs, without and with the blocks' digests, and with the pre-pass skipped;
// `python tests/chain_plan_cases.py FILE [lowered]` writes that plan's own matrix, many-block records among them, in the same
// format (lowered: the cases to run with GPSBB_CHAIN_ONLY_BLOCKS=16 GPSBB_CHAIN_ONLY_LAPS=2000 in the environment).
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -DGPSBB_EXPERIMENTS -Xarch_host -fsanitize=address,undefined \
//         -Ipluto-gps-sim_amd/csrc -Iinclude tools/plan_asan.cpp pluto-gps-sim_amd/csrc/gpsbb_node.cpp -o plan_asan
//   ./plan_asan FILE
// Never loaded into Python, never run on a GPU: nothing here makes a HIP call.
#include "../pluto-gps-sim_amd/csrc/gpsbb.hip"

struct Record { // one set-up; `first`: the case's first push (the carry's rough phases start from zero)
    int32_t nblocks, nch, nsamp, first, opt[5], carry, fixed_prev, carry_prn[GPSBB_MAX_CHAN], fx_prn[GPSBB_MAX_CHAN];
    uint32_t flags, fx_phase[GPSBB_MAX_CHAN];
    double delt;
};

int main(int argc, char **argv)
{
    FILE *f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if (!f)
        return 2;
    Record r;
    double rough[GPSBB_MAX_CHAN] = {0};
    long n = 0;
    while (fread(&r, sizeof r, 1, f) == 1) {
        std::vector<gpsbb_chan_t> ch((size_t)r.nblocks * r.nch);
        if (fread(ch.data(), sizeof(gpsbb_chan_t), ch.size(), f) != ch.size())
            return 3;
        if (r.first)
            memset(rough, 0, sizeof rough);
        double rough0[GPSBB_MAX_CHAN]; // (gpsbb_test_plan advances the rough phases: the launch plans are made from the same ones)
        memcpy(rough0, rough, sizeof rough);
        unsigned long long out[GPSBB_TEST_PLAN_NQ];
        const int rc = gpsbb_test_plan(ch.data(), r.nblocks, r.nch, r.delt, r.nsamp, r.flags, r.opt, r.carry, r.carry ? r.carry_prn : nullptr,
                                       r.carry ? rough : nullptr, r.fixed_prev ? r.fx_prn : nullptr, r.fixed_prev ? r.fx_phase : nullptr, out);
        printf("%d", rc);
        for (int i = 0; rc == GPSBB_OK && i < GPSBB_TEST_PLAN_NQ; i++)
            printf(" %llx", out[i]);
        if ((r.flags & GPSBB_CHAIN_CARRIER) && !(r.flags & GPSBB_FIXED_CARRIER)) { // as a ring's push: the side of its chain, last on the line
            int side[2] = {0, 0};
            const int rs = gpsbb_test_push_side(ch.data(), r.nblocks, r.nch, r.delt, r.nsamp, r.flags, r.opt, side);
            printf(" side %d %d %d", rs, side[0], side[1]);
        }
        printf("\n");
        printf("launch");
        for (int v = 0; v < 5; v++) { // 256 and 8 CUs, without and with digests; then 256 CUs with the pre-pass skipped
            double ph[GPSBB_MAX_CHAN];
            memcpy(ph, rough0, sizeof ph);
            long long lo[GPSBB_TEST_LAUNCH_NQ];
            const int rl = gpsbb_test_launch_plan(ch.data(), r.nblocks, r.nch, r.delt, r.nsamp, r.flags, r.opt, r.carry, r.carry ? r.carry_prn : nullptr,
                                                  r.carry ? ph : nullptr, r.fixed_prev ? r.fx_prn : nullptr, r.fixed_prev ? r.fx_phase : nullptr,
                                                  v == 2 || v == 3 ? 8 : 256, v & 1, v == 4, lo);
            printf(" | %d", rl);
            for (long long i = 0; rl == GPSBB_OK && i < GPSBB_TEST_LAUNCH_NF + 1 + 5 * std::min<long long>(lo[GPSBB_TEST_LAUNCH_NF], GPSBB_TEST_LAUNCH_KERNELS); i++)
                printf(" %lld", lo[i]);
        }
        printf("\n");
        if ((r.flags & GPSBB_CHAIN_CARRIER) && !(r.flags & GPSBB_FIXED_CARRIER)) { // gpsbb_chain_carrier on the same blocks: its plan, a line of its own
            unsigned long long co[GPSBB_TEST_CHAIN_PLAN_NQ];
            const int rc = gpsbb_test_chain_plan(r.nch > 0 ? ch.data() : nullptr, r.nblocks, r.nch, r.delt, r.nsamp, r.opt[0], co);
            printf("chain %d", rc);
            for (unsigned long long i = 0; rc == GPSBB_OK && i < 4 + 4 * std::min<unsigned long long>(co[1], GPSBB_TEST_CHAIN_PLAN_PIECES); i++)
                printf(" %llx", co[i]);
            printf("\n");
        }
        n++;
    }
    fclose(f);
    fprintf(stderr, "plan_asan: %ld set-ups\n", n);
    return 0;
}
