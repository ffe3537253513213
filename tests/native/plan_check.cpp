// plan_check.cpp — the launch planner of ecdna_ssa_ctx_create (ecdna-evo_amd/csrc/ssa_plan.hpp) on the CPU, for
// tests/test_launch_plan.py and tests/test_integration_doc.py. Built for the host alone, with the address and
// undefined-behaviour sanitizers.
//
//   plan_check knobs      prints the planner's knob names, one per line
//   plan_check            reads one case per line from stdin, space-separated key=value words, and prints its plan:
//                         a "plan ..." line and one "chunk ..." line per chunk
//
// A case's words: the parameters the shape is made of (n process flags cell_cap big_cap bin_kmax n_snapshots
// max_workgroups hinted snap_stats passages passage_cells block), the device's facts (cus xccs free occ_rows occ_ref
// occ0 occ1 occ2 occ3) and any knob by its environment name (ECDNA_SSA_ROTATE=1; an empty value leaves the default,
// as in the environment). Unnamed words are 0, block is 256.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "ssa_plan.hpp"

namespace plan = ecdna::plan;

static int run_case(const std::string& line) {
    ecdna_ssa_params_t p{};
    plan::DeviceFacts f;
    plan::Knobs knobs;
    uint64_t snap_stats = 0, passages = 0, passage_cells = 0, block = ecdna::kStepperBlock, hinted = 0;
    static const float kHint = 1.0f;
    std::istringstream words(line);
    std::string w;
    while (words >> w) {
        const size_t eq = w.find('=');
        if (eq == std::string::npos) return std::fprintf(stderr, "plan_check: no '=' in '%s'\n", w.c_str()), 2;
        const std::string key = w.substr(0, eq), text = w.substr(eq + 1);
        int knob = -1;
        for (int k = 0; k < plan::kKnobCount; ++k)
            if (key == plan::kKnobDefs[k].name) knob = k;
        if (knob >= 0) {
            knobs.parse(knob, text.c_str());
            continue;
        }
        const uint64_t v = std::strtoull(text.c_str(), nullptr, 10);
        if (key == "n") p.n_replicates = v;
        else if (key == "process") p.process = (int)v;
        else if (key == "flags") p.flags = (uint32_t)v;
        else if (key == "cell_cap") p.cell_cap = (uint32_t)v;
        else if (key == "big_cap") p.big_cap = (uint32_t)v;
        else if (key == "bin_kmax") p.bin_kmax = (uint32_t)v;
        else if (key == "n_snapshots") p.n_snapshots = (uint32_t)v;
        else if (key == "max_workgroups") p.max_workgroups = (uint32_t)v;
        else if (key == "hinted") hinted = v;
        else if (key == "snap_stats") snap_stats = v;
        else if (key == "passages") passages = v;
        else if (key == "passage_cells") passage_cells = v;
        else if (key == "block") block = v;
        else if (key == "cus") f.cus = (int)v;
        else if (key == "xccs") f.xccs = (int)v;
        else if (key == "free") f.free_bytes = v;
        else if (key == "occ_rows") f.occ_rows = (int)v;
        else if (key == "occ_ref") f.occ_refdraws = (int)v;
        else if (key.size() == 4 && key.compare(0, 3, "occ") == 0 && key[3] >= '0' && key[3] <= '3')
            f.occ_bins[key[3] - '0'] = (int)v;
        else return std::fprintf(stderr, "plan_check: unknown word '%s'\n", w.c_str()), 2;
    }
    p.set_cost_hint = hinted ? &kHint : nullptr;
    plan::RunShape s = plan::run_shape(p, snap_stats != 0, (uint32_t)passages, (uint32_t)passage_cells, knobs);
    s.stepper_block = (uint32_t)block;
    const plan::LaunchPlan pl = plan::plan_launch(s, f, knobs);
    std::printf("plan fits=%d chunk_reps=%llu n_chunks=%zu window=%d schedule=%d stepper_block=%u blocks_cap=%u "
                "rot_tick_log2=%u any_rotation=%d rot_park_min=%d rot_n_pad_max=%llu bin_k=%u bin_c32=%d "
                "row_stride=%llu rep_bytes=%llu snap_rows_local=%d\n",
                pl.chunk_reps ? 1 : 0, (unsigned long long)pl.chunk_reps, pl.chunks.size(), pl.window, pl.schedule,
                pl.stepper_block, pl.stepper_blocks_cap, pl.rot_tick_log2, pl.any_rotation ? 1 : 0, pl.rot_park_min,
                (unsigned long long)pl.rot_n_pad_max, s.bin_k, s.bin_c32, (unsigned long long)s.row_stride,
                (unsigned long long)s.rep_bytes, s.snap_rows_local ? 1 : 0);
    for (const plan::ChunkPlan& ch : pl.chunks) {
        std::printf("chunk first=%llu n=%u blocks=%u rot_n_pad=%u admit_slot=%u admit_remaining=%u rot_parts=",
                    (unsigned long long)ch.first, ch.n, ch.blocks, ch.rot_n_pad, ch.admit_slot, ch.admit_remaining);
        for (uint32_t x = 0; x < ecdna::kRotParts; ++x)
            std::printf("%s%d", x ? "," : "", ch.rot_n_pad ? plan::rot_part_count(ch.n, x) : 0);
        std::printf("\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "knobs") == 0) {
        for (int k = 0; k < plan::kKnobCount; ++k) std::printf("%s\n", plan::kKnobDefs[k].name);
        return 0;
    }
    std::string line;
    while (std::getline(std::cin, line))
        if (int rc = run_case(line)) return rc;
    return 0;
}
