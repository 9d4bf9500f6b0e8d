// The quality gate, the per-frame order and the packed face lists of FaceProcessor.process_numpy on
// gfx950 (fr_quality_gate_device): detections, fit flags and blur scores in HBM become stages,
// metrics, ranks and the list of valid crops in HBM, so the frames -> faces chain reaches the
// embedder without a host hop.
//
// Two launches, one workgroup of 256 threads per frame each.  Nothing here is a throughput kernel:
// a frame has at most FR_GATE_MAX_FACES = 1024 slots of 15 floats, so the work is a few hundred
// scalar operations per slot (the double atan2 / asin dominate) and an all-pairs rank over the
// frame's keys in LDS (8 KiB; every lane of a wave reads the same key, a broadcast).  Fixed
// orders and no atomics: the outputs are a function of the inputs alone.
//
//   gate_rank_kernel   slot i = tid, tid + 256, ...: gate_math.h's gate_slot, the slot's outputs,
//                      its key into LDS; then rank[i] = the number of live slots before it in
//                      process_numpy's stable descending sort; the frame's valid count.
//   gate_pack_kernel   the frame's offsets (sums of the live and valid counts of the frames before
//                      it, block_reduce.h), rows[] by rank, valid_slots[] through an LDS flag array
//                      indexed by rank, and the frame's share of the -1 tails.
#include "block_reduce.h"
#include "gate_math.h"

namespace frhip {

namespace {
constexpr int kThreads = 256;
}

__global__ __launch_bounds__(kThreads) void gate_rank_kernel(GateArgs a) {
  __shared__ double key[FR_GATE_MAX_FACES];
  __shared__ int red[4];
  const int f = blockIdx.x, tid = threadIdx.x, F = a.F;
  const int live = gate_live(a.counts, f, F);
  const long long base = (long long)f * F;
  int valid = 0;
  for (int i = tid; i < F; i += kThreads) {
    const long long slot = base + i;
    GateSlot r;
    if (i < live) {
      r = gate_slot(a.dets + slot * 15, a.ok ? a.ok[slot] : 1, a.lim.check_blur ? a.blur[slot] : 0.0, a.lim);
      key[i] = r.key;
      valid += r.stage == FR_GATE_VALID;
    } else {
      r.stage = FR_GATE_NOT_LIVE;
      r.x0 = r.y0 = r.x1 = r.y1 = 0;
      r.det_score = r.blur_score = r.yaw = r.pitch = r.roll = 0.0;
      a.rank[slot] = -1;
    }
    a.stage[slot] = (uint8_t)r.stage;
    double* m = a.metrics + slot * 5;
    m[0] = r.det_score;
    m[1] = r.blur_score;
    m[2] = r.yaw;
    m[3] = r.pitch;
    m[4] = r.roll;
    int32_t* b = a.bbox + slot * 4;
    b[0] = r.x0;
    b[1] = r.y0;
    b[2] = r.x1;
    b[3] = r.y1;
  }
  valid = block_sum(valid, red);  // its barrier also publishes key[]
  if (tid == 0) a.frame_valid[f] = valid;
  for (int i = tid; i < live; i += kThreads) {
    const double ki = key[i];
    int before = 0;
    for (int j = 0; j < live; ++j) before += gate_before(key[j], j, ki, i);
    a.rank[base + i] = before;
  }
}

__global__ __launch_bounds__(kThreads) void gate_pack_kernel(GateArgs a) {
  __shared__ int slot_at[FR_GATE_MAX_FACES];       // by rank: the slot index within the frame
  __shared__ uint8_t valid_at[FR_GATE_MAX_FACES];  // by rank: the slot is FR_GATE_VALID
  __shared__ int red[4];
  const int f = blockIdx.x, tid = threadIdx.x, F = a.F, n = a.n_frames;
  // live and valid slots of the frames before this one, and of all frames
  int lb = 0, vb = 0, lt = 0, vt = 0;
  for (int g = tid; g < n; g += kThreads) {
    const int l = gate_live(a.counts, g, F), v = a.frame_valid[g];
    lt += l;
    vt += v;
    if (g < f) {
      lb += l;
      vb += v;
    }
  }
  lb = block_sum(lb, red);
  vb = block_sum(vb, red);
  lt = block_sum(lt, red);
  vt = block_sum(vt, red);
  const int live = gate_live(a.counts, f, F), valid = a.frame_valid[f];
  const long long base = (long long)f * F;
  if (tid == 0) {
    a.frame_offsets[f] = lb;
    if (f == 0) {
      a.frame_offsets[n] = lt;
      a.n_valid[0] = vt;
    }
  }
  for (int i = tid; i < live; i += kThreads) {
    const int r = a.rank[base + i];  // a permutation of [0, live): written by gate_rank_kernel
    slot_at[r] = i;
    valid_at[r] = a.stage[base + i] == FR_GATE_VALID;
  }
  __syncthreads();
  for (int r = tid; r < live; r += kThreads) {
    const int slot = (int)base + slot_at[r];
    a.rows[lb + r] = slot;
    if (valid_at[r]) {
      int before = 0;
      for (int q = 0; q < r; ++q) before += valid_at[q] != 0;
      a.valid_slots[vb + before] = slot;
    }
  }
  // the tails: this frame's slots that are not live / not valid, behind those of the frames before it
  const long long dead_at = (long long)lt + (base - lb), invalid_at = (long long)vt + (base - vb);
  for (int k = tid; k < F - live; k += kThreads) a.rows[dead_at + k] = -1;
  for (int k = tid; k < F - valid; k += kThreads) a.valid_slots[invalid_at + k] = -1;
}

hipError_t launch_quality_gate(const GateArgs& a, hipStream_t s) {
  if (a.n_frames < 1 || a.F < 1 || a.F > FR_GATE_MAX_FACES || (long long)a.n_frames * a.F >= (1ll << 31) ||
      !a.dets || !a.stage || !a.metrics || !a.bbox || !a.rank || !a.rows || !a.frame_offsets || !a.valid_slots ||
      !a.n_valid || !a.frame_valid || (a.lim.check_blur && !a.blur))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(gate_rank_kernel, dim3((unsigned)a.n_frames), dim3(kThreads), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(gate_pack_kernel, dim3((unsigned)a.n_frames), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace frhip
