// ce_host.cpp -- host side of the CE object: target checks and staging, launch, running totals, progress and report text.
// Replaces eesen::CE::EvalParallel / Eval / Report (the reference's src/net/ce-loss.cc:30-175).  The arithmetic is in ce.hip.
#include <algorithm>
#include <cmath>
#include <limits>
#include <sstream>

#include "net.h"

namespace eesen {

CeLoss::CeLoss(int dev, void* stream) : device(dev) {
  require_device(dev);
  st = reinterpret_cast<hipStream_t>(stream);  // NULL = the device's default stream (shared with the Net)
}

CeLoss::~CeLoss() {   // drained here; the guard hook, the pinned slots and the events go with the members
  (void)hipSetDevice(device);
  (void)hipStreamSynchronize(st);
}

// The totals and the progressive report of ce-loss.cc:144-167, in call order.  obj_out (may be null): this call's objective.
void CeLoss::fold(Pending& q, double* obj_out) {
  if (!q.active) return;
  q.pin.wait();
  q.active = false;
  const CeSums* r = q.pin.as<CeSums>();
  if (StatGuard::raised(r, sizeof(CeSums))) {  // computed from a timed-out forward pass (StatGuard): not a statistic
    if (obj_out) *obj_out = std::numeric_limits<double>::quiet_NaN();
    guard.note_dropped("CE");
    return;
  }
  const double ce = r->obj;
  if (obj_out) *obj_out = ce;
  obj += ce;
  obj_progress += ce;
  correct += r->correct;
  correct_progress += r->correct;
  sequences_progress += q.S;
  sequences += q.S;
  frames_progress += q.rows;   // num_frames = net_out.NumRows(): padded rows count (:102, :148-149)
  frames += q.rows;
  if (sequences_progress > report_step) {   // :153-167, the reference's text byte for byte (no space before "Frame-level")
    std::ostringstream os;
    os << "After " << sequences << " sequences (" << frames / (100.0 * 3600) << "Hr): "
       << "CE-Obj = " << obj_progress / sequences_progress
       << "Frame-level CE-Obj = " << obj_progress / frames_progress
       << "   FrameAcc = " << 100.0 * (double(correct_progress) / frames_progress) << "%"
       << " obj_progress_=  " << obj_progress
       << " sequences_progress_=  " << sequences_progress
       << " frames_progress_=  " << frames_progress;
    progress.push_back(os.str());
    sequences_progress = 0;
    frames_progress = 0;
    obj_progress = 0.0;
    correct_progress = 0;
  }
}

void CeLoss::flush() {
  EESEN_HIP_CHECK(hipSetDevice(device));
  for (unsigned k = 0; k < 2; ++k) fold(pend[(pend_idx + k) & 1], nullptr);   // oldest first
}

void CeLoss::eval_parallel(const int* frame_num_utt, int S, const float* net_out, int rows, int K, int ld, const int* targets,
                           float* diff, int ldd, double* obj_host) {
  check_shape(frame_num_utt, S, rows, K, ld, 1);
  EESEN_REQUIRE(ldd >= K, EESEN_ERR_INVALID, "leading dimension smaller than the class count");
  const int T = rows / S;
  // ce-loss.cc:106-113 checks every row's id (an id of a padded row is 0 there); only the valid rows' ids are read here, and a
  // negative one -- an out-of-bounds write in the reference -- is refused as well
  for (int t = 0; t < T; ++t)
    for (int s = 0; s < S; ++s) {
      if (t >= frame_num_utt[s]) continue;
      const int id = targets[(size_t)t * S + s];
      if (id < 0 || id >= K)
        throw Error(EESEN_ERR_INVALID, "Class id out of network output dimension. Net outputs: " + std::to_string(K) +
                                           ", class ID : " + std::to_string(id));
    }
  EESEN_HIP_CHECK(hipSetDevice(device));

  // lens + targets: one stream-ordered upload (StageSlots)
  const size_t n = (size_t)S + rows;
  const int nb = ce_eval_blocks(rows);
  if (tg.cap < n || part.cap < (size_t)nb || res.cap < 1) EESEN_HIP_CHECK(hipStreamSynchronize(st));  // reallocation frees what queued kernels may read
  tg.reserve(n);
  part.reserve(nb);
  res.reserve(1);
  stage.upload(st, tg.p, n, [&](int* pinned) {
    std::copy(frame_num_utt, frame_num_utt + S, pinned);
    std::copy(targets, targets + rows, pinned + S);
  });

  clock.mark(st, 0);
  ce_eval(st, net_out, ld, rows, K, S, tg.p, tg.p + S, diff, ldd, part.p, res.p);
  clock.stop(st);

  // the sums (and the guard word's value when they were computed) back through a pinned slot
  Pending& q = pend[pend_idx++ & 1];
  fold(q, nullptr);
  guard.read_back(q.pin, res.p, sizeof(CeSums), st);
  q.S = S; q.rows = rows; q.active = true;
  if (obj_host) {
    fold(pend[pend_idx & 1], nullptr);   // the older one first: totals accumulate in call order
    fold(q, obj_host);
  }
}

// CE::Report (ce-loss.cc:171-175) with one deliberate change: the reference divides two int32 (correct_ / frames_), so it only
// ever prints 0 or 100 (or divides by zero); this is the true ratio in the same shape.
std::string CeLoss::report() {
  flush();
  std::ostringstream oss;
  oss << "\nFRAME_ACCURACY >> " << 100.0 * (double(correct) / double(frames)) << "% <<";
  return oss.str();
}

}  // namespace eesen
