// vaa_rows.h — row-statistics records of K3's ROWS path, shared by vaa_loss.hip (K3) and vaa_head.hip (LM head fused with K3's statistics).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace vaa {

constexpr int kA0 = 31744;  // first action token (UADA.py:384)
constexpr int kNA = 256;    // action bins

struct RowMap {  // one per labelled position, in (b,k) row-major order of labels[b,k+1] != -100 (vaa_loss_rowmap_build)
    int b, k, lab, ord;
};
struct PartStat {  // one per (row, part)
    float m, s;    // max and sum exp(z - m) over the part
    float zlab;    // logit of the label if it lies in this part, else -inf
    int amax;      // argmax over the part (global column index), lowest index on ties
};
struct SliceStat {  // one per row
    float alse, E;
    int pred;
    int pad;
};

int rows_split(int R, int V);

// SEGMENTED row map (vaa_loss_rowmap_build_seg: P groups of Bp consecutive images, one maskidx sweep group each), int words:
//   [0, 4)        {R, #action rows of all groups, P, Bp}             (an ordinary map has {R, #action rows, 0, 0})
//   [4, T)        RowMap[R] of the whole batch, exactly the ordinary map's rows; T = rowmap_seg_table(B, L)
//   [T, T + 4P)   per group {first row, rows, action rows, 0}
//   [S_g, ...)    group g's own ordinary map {R_g, nact_g, 0, 0} + RowMap[R_g] (image index within the group): S_g = rowmap_seg_sub(B, L, P, g)
// The group's own map is what vaa_step_epilogue_seg folds with: bit for bit the fold a standalone run of that group performs.
inline __host__ __device__ int rowmap_seg_table(int B, int L) { return 4 + 4 * B * (L - 1); }
inline __host__ __device__ int rowmap_seg_sub(int B, int L, int P, int g) { return rowmap_seg_table(B, L) + 4 * P + g * (4 + 4 * (B / P) * (L - 1)); }
// word w of image b's group in a segmented map's table (1: rows, 2: action rows) — on an ordinary map the header's count of the whole batch
__device__ __forceinline__ int row_group_word(const int* rowmap, int tbl, int b, int w) {
    const int P = rowmap[2];
    if (P <= 0) return rowmap[w - 1];
    const int Bp = rowmap[3] > 0 ? rowmap[3] : 1;
    int g = b / Bp;
    g = g < 0 ? 0 : (g >= P ? P - 1 : g);
    return rowmap[tbl + 4 * g + w];
}
// the count that normalises row b's gradient (the kE term of UADA_ddp.py:99-124's mean over action rows): its group's on a segmented map
__device__ __forceinline__ int row_action_count(const int* rowmap, int tbl, int b) { return row_group_word(rowmap, tbl, b, 2); }
// ... and the one of the cross-entropy mean over ALL labelled rows (TMA.py:148): the rows of its group
__device__ __forceinline__ int row_label_count(const int* rowmap, int tbl, int b) { return row_group_word(rowmap, tbl, b, 1); }

// head workspace of vaa_head_loss_rows_stats: [R][ceil(V / 128)] PartStat, then (256-byte aligned) the action-column logits [R][256] bf16
constexpr int kHeadCols = 128;  // vocabulary columns per workgroup of head_stats_kernel
inline size_t head_ws_align(size_t n) { return (n + 255) / 256 * 256; }
inline size_t head_ws_slice_offset(int R, int V) { return head_ws_align((size_t)R * ((V + kHeadCols - 1) / kHeadCols) * sizeof(PartStat)); }  // parts per row of the K3 workspace layout [R][4] PartStat + [R] SliceStat (vaa_loss.hip)

}  // namespace vaa
