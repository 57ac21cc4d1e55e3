// kfstore_math.h — a keyframe's feature grid by the keyframe's own rule, host + device: KeyFrame::PosInGrid (cslam/src/KeyFrame.cpp:265-275) and the order
// KeyFrame::AssignFeaturesToGrid (:206-225) leaves inside a cell.  The rule reads mvKeysUn, the int bounds mnMinX / mnMinY and the two grid inverses alone, all of
// which the keyframe keeps and serialises, so a keyframe born from a message has exactly this grid.  (A Frame-born keyframe's grid is the Frame's, built from the
// Frame's float bounds: frame_math.h frame_cell_of.)  The grid kernel of kfstore.hip runs these lines; cslam::KeyFrameStore (host/ccm_host.cpp) compiles them
// with g++.  The argument rules of ccm_kfstore_add follow.  Compile with -ffp-contract=off: the difference and the product are two roundings.
#pragma once
#include "fuse_math.h"

#define KFG_MAX_FEAT 65535    // cell_idx is 16 bits wide and FSM_NO_IDX is no feature
#define KFG_FEAT_ALIGN 16     // a slot's stride in features is a multiple of this: its descriptors, xy, octaves and cell_idx all start on 16 bytes

// KeyFrame::PosInGrid for the keypoint (x, y) of a keyframe with the record rec (rec[4], rec[5]: the floats of mnMinX, mnMinY; rec[8], rec[9]: the inverses).
// true and the cell posX * 48 + posY (x-major, as fuse_math.h reads it) when the keypoint is in the grid.  round(float) is half away from zero.  A product that no
// int holds (NaN, Inf, beyond the int range) is undefined in the source (x86 gives INT_MIN, which is < 0); stated here as "not in the grid" so that host and device
// agree.  Every |t| < 2^31 rounds to a float that an int holds, and the range test below needs far less.
FSM_HD bool kfg_cell_of(const float rec[FSM_REC_FLOATS], float x, float y, int* cell) {
  const float tx = (x - rec[4]) * rec[8], ty = (y - rec[5]) * rec[9];
  if (!(tx > -1.0f && tx < (float)FSM_GRID_COLS) || !(ty > -1.0f && ty < (float)FSM_GRID_ROWS)) return false;   // NaN fails both; roundf of anything else is outside
  const int posX = (int)roundf(tx), posY = (int)roundf(ty);
  if (posX < 0 || posX >= FSM_GRID_COLS || posY < 0 || posY >= FSM_GRID_ROWS) return false;
  *cell = posX * FSM_GRID_ROWS + posY;
  return true;
}

// max_feat rounded up to the slot stride; 0 when it is outside 1 .. KFG_MAX_FEAT
FSM_HD int kfg_stride(int max_feat) {
  if (max_feat < 1 || max_feat > KFG_MAX_FEAT) return 0;
  return (max_feat + KFG_FEAT_ALIGN - 1) / KFG_FEAT_ALIGN * KFG_FEAT_ALIGN;
}

// AssignFeaturesToGrid for one keyframe on the calling thread: cell_off[FSM_CELLS + 1] (exclusive prefix, ends at the features in the grid) and cell_idx (the
// features of a cell in ascending order: the reference's push_back order).  A counting sort in two passes over the features.  Returns n_in.
FSM_HD int kfg_build_host(const float rec[FSM_REC_FLOATS], int n, const float* xy, int32_t* cell_off, uint16_t* cell_idx) {
  for (int c = 0; c <= FSM_CELLS; c++) cell_off[c] = 0;
  int cell;
  for (int f = 0; f < n; f++)
    if (kfg_cell_of(rec, xy[2 * f], xy[2 * f + 1], &cell)) cell_off[cell + 1]++;
  for (int c = 0; c < FSM_CELLS; c++) cell_off[c + 1] += cell_off[c];
  // cell_off[c] serves as cell c's cursor and is moved back afterwards
  for (int f = 0; f < n; f++)
    if (kfg_cell_of(rec, xy[2 * f], xy[2 * f + 1], &cell)) cell_idx[cell_off[cell]++] = (uint16_t)f;
  for (int c = FSM_CELLS; c > 0; c--) cell_off[c] = cell_off[c - 1];
  cell_off[0] = 0;
  return cell_off[FSM_CELLS];
}

// The argument rules of ccm_kfstore_add that read the arrays alone (the keys and the free slots are the store's to check); nullptr, or what is wrong.  A supplied
// grid is held to ccm_fuse_sim3_eval's rules, except that it may end below the keyframe's feature count (a Frame's grid leaves out the keypoints outside it); its
// cell_idx then has cell_off[FSM_CELLS] entries at feat_off[m].
FSM_HD const char* kfg_check_add(int M, int max_feat, const float* kf_rec, const int32_t* feat_off, const float* feat_xy, const uint8_t* feat_octave,
                                 const uint8_t* feat_desc, const int32_t* cell_off, const int32_t* cell_idx) {
  if (M < 0) return "M negative";
  if (M == 0) return nullptr;
  if (!kf_rec || !feat_off) return "null pointers";
  if ((cell_off == nullptr) != (cell_idx == nullptr)) return "cell_off and cell_idx are both NULL or both given";
  if (feat_off[0] != 0) return "feat_off[0] != 0";
  for (int m = 0; m < M; m++) {
    const int64_t n = (int64_t)feat_off[m + 1] - feat_off[m];
    if (n < 0) return "feat_off decreases";
    if (n > (int64_t)max_feat) return "a keyframe with more than max_feat features";
  }
  if (feat_off[M] && (!feat_xy || !feat_octave || !feat_desc)) return "null pointers";
  if (!cell_off) return nullptr;
  for (int m = 0; m < M; m++) {
    const int32_t n = feat_off[m + 1] - feat_off[m];
    const int32_t* co = cell_off + (size_t)m * (FSM_CELLS + 1);
    if (co[0] != 0) return "cell_off does not start at 0";
    for (int c = 0; c < FSM_CELLS; c++)
      if (co[c + 1] < co[c]) return "cell_off decreases";
    if (co[FSM_CELLS] > n) return "cell_off ends beyond the keyframe's feature count";
    if (co[FSM_CELLS] && !cell_idx) return "null pointers";
    const int32_t* ci = cell_idx + feat_off[m];
    for (int32_t j = 0; j < co[FSM_CELLS]; j++)
      if (ci[j] < 0 || ci[j] >= n) return "cell_idx out of range";
  }
  return nullptr;
}
