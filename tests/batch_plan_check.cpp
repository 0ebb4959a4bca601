// csrc/cmax_batch_plan.h on its own (tests/test_batch_plan_host.py): reads cases from the file named on the command line, runs
// cut_work_list / radix_pass_plan on each and prints one line of integers per case.  No other file of the library, no HIP.
//   in : cut <ntr> <ntc> <n_time_bin> <slab_major> <n> <long_runs> <big> <mid> <small_acc> <free_cut> <seg_cap> <no_owned> <compact> <group_start x (ngroups + 1)>
//   out: cut <status> <big> <mid> <owned> <small_acc> <wants_compact> <seg_max> <nseg> <nrows> <first count group0 ngroups x nseg> <row_seg_start x nrows>
//   in : plan <ntiles> <n_time_bin> <n_in> <digit_bits>
//   out: plan <planned> <P> <fine> <nwg> <range> <need> <nb x P> <sh x P>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../event_based_optical_flow_amd/csrc/cmax_batch_plan.h"

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: batch_plan_check <cases.txt>\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    std::string kind;
    long cases = 0;
    while (in >> kind) {
        if (kind == "cut") {
            int ntr, ntc, T, slab, long_runs, no_owned, compact;
            long long n;
            cmax::CutKnobs k;
            in >> ntr >> ntc >> T >> slab >> n >> long_runs >> k.big >> k.mid >> k.small_acc >> k.free_cut >> k.seg_cap >> no_owned >> compact;
            k.no_owned = no_owned != 0;
            k.compact = compact != 0;
            std::vector<int> gs((size_t)ntr * ntc * (T > 0 ? T : 1) + 1);
            for (int &v : gs) in >> v;
            if (!in) break;
            const cmax::WorkList wl = cmax::cut_work_list(gs.data(), ntr, ntc, T, slab != 0, n, long_runs != 0, k);
            std::cout << "cut " << (int)wl.status << ' ' << wl.big << ' ' << wl.mid << ' ' << wl.owned << ' ' << wl.small_acc << ' ' << wl.wants_compact << ' '
                      << wl.seg_max << ' ' << wl.segs.size() << ' ' << wl.row_seg_start.size();
            for (const cmax::Segment &s : wl.segs) std::cout << ' ' << s.first << ' ' << s.count << ' ' << s.group0 << ' ' << s.ngroups;
            for (int r : wl.row_seg_start) std::cout << ' ' << r;
            std::cout << '\n';
        } else if (kind == "plan") {
            int ntiles, T, bits;
            long long n_in;
            in >> ntiles >> T >> n_in >> bits;
            if (!in) break;
            const cmax::RadixPlan p = cmax::radix_pass_plan(ntiles, T, n_in, bits);
            std::cout << "plan " << p.planned << ' ' << p.P << ' ' << p.fine << ' ' << p.nwg << ' ' << p.range << ' ' << p.need;
            for (int q = 0; q < p.P; ++q) std::cout << ' ' << p.nb[q];
            for (int q = 0; q < p.P; ++q) std::cout << ' ' << p.sh[q];
            std::cout << '\n';
        } else {
            std::fprintf(stderr, "unknown case kind '%s'\n", kind.c_str());
            return 2;
        }
        ++cases;
    }
    if (!in.eof()) {
        std::fprintf(stderr, "malformed case file after %ld cases\n", cases);
        return 2;
    }
    std::cout << "done " << cases << '\n';
    return 0;
}
