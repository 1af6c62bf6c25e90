// ev_carr_log2 (csrc/gpsbb_events.hip.h), the host side of the per-kind state granule, under the host sanitizers on a machine
// without a GPU: the rule for every g the knob admits and beyond, the carrier row's bounds as the table digest indexes them, and
// ev_state_at / ev_states_used, which every reader and writer of the tile tables goes by.
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
    /* the rule every reader and writer of the tile tables goes by (ev_state_at, ev_states_used): the entry is one the kind's row
     * uses, entry and tiles-since give the tile back, and both are what the kernels had written out by hand */
    for (int g = 0; g <= EV_STATE_LOG2_MAX; g++)
        for (int kind = NCO_CODE; kind <= NCO_CARR; kind++)
            for (int ntiles = 1; ntiles <= 70; ntiles++) {
                const int gk = kind == NCO_CARR ? ev_carr_log2(g) : g, used = ev_states_used(g, kind, ntiles);
                std::vector<int> row((size_t)used, 0);
                for (int t = 0; t < ntiles; t++) {
                    const EvStateAt at = ev_state_at(g, kind, t);
                    row[(size_t)at.entry]++; /* (out of bounds here is the sanitizer's to report) */
                    bad += at.entry < 0 || at.entry >= used || (at.entry << at.log2) + at.since != t;
                    bad += at.log2 != gk || at.entry != t >> gk || at.since != (t & ((1 << gk) - 1));
                }
                for (int k = 0; k < used; k++)
                    bad += row[(size_t)k] < 1 || row[(size_t)k] > 1 << gk;
                bad += used != (ntiles + (1 << gk) - 1) >> gk || used > ev_states_used(g, NCO_CODE, ntiles);
                bad += ev_tile_x_row(3, 5, 2, kind, used) != (size_t)((3 * 2 * 5 + 2 * 2 + kind) * used);
                bad += ev_tile_nav_row(3, 5, 2, used) != (size_t)((3 * 5 + 2) * used);
            }
    printf("granule_asan: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
