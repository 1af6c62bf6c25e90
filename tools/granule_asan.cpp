// ev_carr_log2 (csrc/gpsbb_events.hip.h), the host side of the per-kind state granule, under the host sanitizers on a machine
// without a GPU: the rule for every g the knob admits and beyond, and the carrier row's bounds as the table digest indexes them.
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -DGPSBB_EXPERIMENTS -Xarch_host -fsanitize=address,undefined \
//         -Ipluto-gps-sim_amd/csrc -Iinclude tools/granule_asan.cpp pluto-gps-sim_amd/csrc/gpsbb_node.cpp -o granule_asan
//   ./granule_asan
// Never loaded into Python, never run on a GPU: nothing here makes a HIP call.
#include "../pluto-gps-sim_amd/csrc/gpsbb.hip"

int main()
{
    int bad = 0;
    for (int g = -3; g <= EV_STATE_LOG2_MAX + 3; g++) {
        const int gc = ev_carr_log2(g);
        const int want = g >= 1 ? (g + 1 < EV_STATE_LOG2_MAX ? g + 1 : EV_STATE_LOG2_MAX) : 0;
        printf("g %d gc %d\n", g, gc);
        bad += gc != want || !ev_carr_granule_fits(gc);
    }
    /* a carrier row uses the first ceil(ntiles / 2^gc) of the nstates = ceil(ntiles / 2^g) entries its stride gives it */
    for (int g = 0; g <= EV_STATE_LOG2_MAX; g++)
        for (int ntiles = 1; ntiles <= 70; ntiles++) {
            const int gc = ev_carr_log2(g), nst = (ntiles + (1 << g) - 1) >> g, nsty = (ntiles + (1 << gc) - 1) >> gc;
            std::vector<int> row((size_t)nst, 0);
            for (int t = 0; t < ntiles; t += 1 << gc)
                row[(size_t)(t >> gc)]++; /* (out of bounds here is the sanitizer's to report) */
            for (int k = 0; k < nst; k++)
                bad += row[(size_t)k] != (k < nsty ? 1 : 0);
            bad += nsty > nst || gc < g;
        }
    printf("granule_asan: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
