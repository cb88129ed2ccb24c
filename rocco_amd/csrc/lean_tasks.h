// rocco_amd/csrc/lean_tasks.h -- how the host fills the descriptors of lean.h and lays out the buffers they travel in.
// Plain C++ (no HIP call): budget.hip uses it for every round, tests/host_logic/harness.cpp checks the layouts on the CPU.
#pragma once

#include <cmath>
#include <vector>

#include "model_chain.h"

namespace rocco {

inline int lean_tiles(size_t n) { return (int)((n + kLeanTile - 1) / kLeanTile); }

// What tells the kinds of LeanTask apart; everything else follows from the level and the problem.
struct LeanTaskKind {
    int batch = kLeanBatch;
    int store = 0;
    long long bits_begin = 0, off_begin = 0;
    int tile_stride = 1, independent = 0;
    const uint8_t *emap = nullptr;
    const double *wcap = nullptr;
    const unsigned *clean_chunks = nullptr;
    double cmax = 0.0, sabs = 0.0;

    // bound evaluation of a level whose kept-locus words and tile offsets are stored (word offsets into the level pool)
    static LeanTaskKind bound_stored(long long bits_begin, long long off_begin)
    {
        LeanTaskKind k;
        k.store = 1;
        k.bits_begin = bits_begin;
        k.off_begin = off_begin;
        return k;
    }
    // every stride-th tile of the array, each as a chain of its own; nothing is kept
    static LeanTaskKind pilot(int stride)
    {
        LeanTaskKind k;
        k.tile_stride = stride;
        k.independent = 1;
        return k;
    }
    // the reference's own arithmetic from the binade map (lean_model_kernel)
    static LeanTaskKind model(const uint8_t *emap, const double *wcap, const unsigned *clean_chunks, double cmax, double sabs)
    {
        LeanTaskKind k;
        k.batch = kLeanModelBatch;
        k.emap = emap;
        k.wcap = wcap;
        k.clean_chunks = clean_chunks;
        k.cmax = cmax;
        k.sabs = sabs;
        return k;
    }
    // the binade map of a level (lean_map_kernel): one penalty, one workgroup per tile
    static LeanTaskKind map()
    {
        LeanTaskKind k;
        k.batch = 1;
        return k;
    }
};

// A task over the level (s, m) of a problem with switch cost `gamma` on the grid 2^qexp, `n_points` penalties.  The cursors
// of its round (unit_begin, point_begin, rec_begin, result_begin) are zero: the caller's.
inline LeanTask lean_task(const double *s, long long m, double gamma, int qexp, const LeanTaskKind &k, int n_points)
{
    LeanTask t = {};
    t.s = s;
    t.m = m;
    t.c_raw = gamma;
    t.magic = std::ldexp(1.5, 52 + qexp);
    t.big = std::ldexp(1.0, 50 + qexp);
    t.n_tiles = (lean_tiles((size_t)m) + k.tile_stride - 1) / k.tile_stride;
    t.n_points = n_points;
    t.n_groups = (n_points + k.batch - 1) / k.batch;
    t.bits_begin = k.bits_begin;
    t.off_begin = k.off_begin;
    t.tile_stride = k.tile_stride;
    t.independent = k.independent;
    t.store = k.store;
    t.emap = k.emap;
    t.wcap = k.wcap;
    t.clean_chunks = k.clean_chunks;
    t.cmax = k.cmax;
    t.sabs = k.sabs;
    t.qexp = qexp;
    t.batch = k.batch;
    return t;
}

// Where a problem's tolerance cap lives (dev_lean_wcap): the value, the 384 counters it is summed from, the clean-chunk table.
struct LeanWcapSlot {
    double *wcap;
    unsigned *counters;
    unsigned *clean_chunks;
};

inline LeanWcapSlot lean_wcap_slot(void *base, size_t n_problems, size_t problem)
{
    LeanWcapSlot slot;
    slot.wcap = (double *)base + problem;
    slot.counters = (unsigned *)((char *)base + align_up(n_problems * sizeof(double), 256)) + 512 * problem;
    slot.clean_chunks = slot.counters + 384;
    return slot;
}

inline LeanWcapTask lean_wcap_task(const uint8_t *emap, const double *s, long long m, int qexp, double cmax, double sabs,
                                   const LeanWcapSlot &slot, int block_begin)
{
    LeanWcapTask wt;
    wt.emap = emap;
    wt.s = s;
    wt.m = m;
    wt.qexp = qexp;
    wt.e_floor = std::ilogb(2.0 * cmax + 2.0 * sabs + (sabs + 2.0) + 2.0);  // (|penalty| <= sabs + 2)
    wt.counters = slot.counters;
    wt.clean_chunks = slot.clean_chunks;
    wt.wcap = slot.wcap;
    wt.block_begin = block_begin;
    wt.pad = 0;
    return wt;
}

// Penalties per workgroup: a workgroup's time grows with what it carries (about 6 us + 4 us per penalty), a round's with
// the number of waves of workgroups the device needs (512 at a time).  While the whole round fits at once, carry less per
// workgroup (`full`: what the tasks carry now).
inline void lean_rebatch(std::vector<LeanTask> &ts, int full, int &total_units)
{
    for (int b = 2; b < full; b *= 2) {
        long long u = 0;
        for (const LeanTask &t : ts) {
            u += (long long)t.n_tiles * ((t.n_points + b - 1) / b);
        }
        if (u <= 512) {
            int at = 0;
            for (LeanTask &t : ts) {
                t.batch = b;
                t.n_groups = (t.n_points + b - 1) / b;
                t.unit_begin = at;
                at += t.n_tiles * t.n_groups;
            }
            total_units = at;
            return;
        }
    }
}

// The three buffers of a chain of rounding-model rounds (model_chain.h) over B problems, of which n_wcap need their
// tolerance cap computed first; `cap_pairs` (tile, penalty) pairs per round keep solution words.
//   device:        [tasks][walk][wcap tasks] (uploaded) [state][points][results][ctl][globals][writes][n_writes][entering][bits]
//   pinned upload: the uploaded prefix, same offsets
//   host-coherent: [report][n_points per round and problem][finals][facts]
struct ModelChainLayout {
    size_t tasks, walk, wcap, up_bytes;
    size_t state, points, results, ctl, globals, writes, n_writes, entering, bits, dev_bytes;
    size_t report, n_points, finals, facts, follow_bytes;
};

inline ModelChainLayout model_chain_layout(size_t B, size_t n_wcap, int rounds, long long cap_pairs)
{
    ModelChainLayout m;
    Layout dev;
    m.tasks = dev.at(B * sizeof(LeanTask));
    m.walk = dev.at(B * sizeof(ModelChainWalk));
    m.wcap = dev.at(n_wcap * sizeof(LeanWcapTask));
    dev.end_upload();
    m.up_bytes = dev.uploaded;
    m.state = dev.at(B * sizeof(ModelChainState));
    m.points = dev.at(B * kLeanMaxPoints * sizeof(double));
    m.results = dev.at(B * kLeanMaxPoints * sizeof(LeanResult));
    m.ctl = dev.at(sizeof(LeanRoundCtl));
    m.globals = dev.at(3 * sizeof(int));
    m.writes = dev.at(B * sizeof(LeanWriteTask));
    m.n_writes = dev.at(sizeof(int));
    // what writes the final solutions at the chain's end (lean.h: LeanTask::store == 2): one entering value and two
    // 256-word planes per (tile, penalty) pair of every round
    m.entering = dev.at((size_t)rounds * (size_t)cap_pairs * sizeof(unsigned));
    m.bits = dev.at((size_t)rounds * (size_t)cap_pairs * 2 * 256 * sizeof(unsigned));
    m.dev_bytes = dev.bytes();
    Layout follow;
    m.report = follow.at(sizeof(ModelChainReport));
    m.n_points = follow.at((size_t)rounds * B * sizeof(int));
    m.finals = follow.at(B * sizeof(ModelChainFinal));
    m.facts = follow.at((size_t)rounds * B * kLeanMaxPoints * sizeof(ModelChainFact));
    m.follow_bytes = follow.bytes();
    return m;
}

}  // namespace rocco
