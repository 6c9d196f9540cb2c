// What the int8-MFMA deployment blocks share (qgemm_codes_mfma.h, qgemm_bits_mfma.h, qgemm_iao8.h): the SET / tile table their packers build, and the rule that sizes
// the launch grid of every bit / code / byte forward.
//
//   set / tile table : the output positions are cut into SETS of 64 consecutive positions, the unit a wave of the forward kernel assembles on chip.  The rows of a set
//                      are sorted by group and cut into TILES of 16 inside a group (the rows of a tile share the B operand of mn_mfma_i8); a set has at most `slots`
//                      tiles, and the table holds, behind the form's own header words, one tile COUNT per set (at the form's count offset) and then, 16-byte aligned
//                      at `tiles_off`, `slots` tiles of `tstride` words per set.  Slots past the count, and the rows of a tile past its group's last, are DEAD rows: how
//                      a dead row reads (a threshold never met, no destination) is the form's business, as are the tile's metadata, the weight bytes and the header.
//                      Row j of the table computes channel out_order[j] (the consumer's channel shuffle folded into its producer); positions >= O and bad out_order
//                      entries have no row at all, and the bad entries are counted into a header word the form names.
//   grid             : grid.x = the pixel blocks; grid.y deals the form's units (sets, output words, spans) where the pixels alone do not fill the chip.
#pragma once
#include "qgemm_dev.h"

namespace mn_sets {

enum { SETROWS = 64 };

// ---------------------------------------------------------------- host: the launch grid
// grid.y for bx pixel blocks and `units` to deal over it
static inline int grid_rows(int bx, int units) {
    const int gy = (2048 + bx - 1) / bx;          // enough blocks to fill the chip: split the units over grid.y when the pixels alone do not
    return gy < units ? gy : units;
}
// ... where a block takes `per` consecutive units: no block of grid.y is left without one
static inline int grid_deal(int bx, int units, int& per) {
    const int gy = grid_rows(bx, units);
    per = (units + gy - 1) / gy;
    return (units + per - 1) / per;
}

// ---------------------------------------------------------------- host: the tile table of a geometry G { nsets, slots, tstride, tiles_off }
template <class G>
static inline int64_t table_words(const G& m) { return (int64_t)m.tiles_off + (int64_t)m.nsets * m.slots * m.tstride; }

// m.nsets and m.tstride are set: fills m.slots and m.tiles_off (the per-set counts stand at cnt_off); false: the table would not stay below 2^30 words
template <class G>
static inline bool table_layout(G& m, int groups, int cnt_off) {
    const int gp = groups < SETROWS ? groups : SETROWS;
    m.slots = (SETROWS + 15 * gp) / 16;          // sum over the groups of a set of ceil(rows / 16), at most
    m.tiles_off = (cnt_off + m.nsets + 3) & ~3;
    return table_words(m) < (1ll << 30);
}

// ---------------------------------------------------------------- device: the rows of one set placed into tiles (a block of at least SETROWS threads per set)
struct SetPlan {
    int chan[SETROWS], grp[SETROWS], tile[SETROWS], row[SETROWS];          // per position: its channel (-1: no row), its group, its tile in the set and its row in the tile
    int cnt[SETROWS], first[SETROWS];                                      // (scratch: the rows of the position's group, 1 at the group's first position)
    int off[SETROWS];                                                      // set by a packer for a row with a weight off its grid (plan_set clears it, tally_off sums it)
};

// Called by the whole block uniformly (barriers inside, the last one behind the last write to `s`).  Fills s.chan, s.grp, s.tile, s.row; counts the bad out_order entries
// into *bad; returns this thread's number of rows of its group in front of it (before >> 4 == 0: its tile is the first of its group in the set).  ntiles: the set's
// tile count, in thread 0 (0 elsewhere), which the caller stores where its table keeps it.
__device__ __forceinline__ int plan_set(const int32_t* __restrict__ order, int O, int Og, int set, uint32_t* bad, SetPlan& s, int& ntiles) {
    const int tid = threadIdx.x;
    ntiles = 0;
    // the channel and group of every position of the set (a bad out_order entry -- counted -- or a position past O: no row)
    if (tid < SETROWS) {
        const int jj = set * SETROWS + tid;
        int o = jj < O ? (order ? order[jj] : jj) : -1;
        o = (o >= 0 && o < O) ? o : -1;
        s.chan[tid] = o; s.grp[tid] = o < 0 ? INT_MAX : o / Og; s.off[tid] = 0;
        if (jj < O && o < 0) atomicAdd(bad, 1u);
    }
    __syncthreads();
    int before = 0;
    if (tid < SETROWS) {
        int cnt = 0;
        for (int jj = 0; jj < SETROWS; ++jj) {
            const int same = s.chan[jj] >= 0 && s.grp[jj] == s.grp[tid];
            cnt += same; before += same && jj < tid;
        }
        s.cnt[tid] = cnt; s.first[tid] = s.chan[tid] >= 0 && before == 0;
    }
    __syncthreads();
    if (tid < SETROWS) {
        int tb = 0;          // tiles of the groups in front of this row's
        for (int jj = 0; jj < SETROWS; ++jj)
            if (s.first[jj] && s.grp[jj] < s.grp[tid]) tb += (s.cnt[jj] + 15) >> 4;
        s.tile[tid] = tb + (before >> 4); s.row[tid] = before & 15;
        if (tid == 0)
            for (int jj = 0; jj < SETROWS; ++jj)
                if (s.first[jj]) ntiles += (s.cnt[jj] + 15) >> 4;
    }
    __syncthreads();
    return before;
}

// the rows of the set a packer has flagged in s.off, added to *counter (whole block, uniformly)
__device__ __forceinline__ void tally_off(const SetPlan& s, uint32_t* counter) {
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t nbad = 0;
        for (int i = 0; i < SETROWS; ++i) nbad += (uint32_t)(s.off[i] != 0);
        if (nbad) atomicAdd(counter, nbad);
    }
}

}  // namespace mn_sets
