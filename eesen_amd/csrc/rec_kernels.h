// rec_kernels.h -- what lstm_persistent.hip exports to the planner (rec_plan.cpp): ONE table of its instantiations, a row each.
// A row's name is the stringised text of the very tokens that take its host stub's address, so the name a plan reports and the
// kernel it launches cannot disagree.  Occupancy query, resource query, census and launch all go through the row's address
// (hipOccupancyMaxActiveBlocksPerMultiprocessor / hipFuncGetAttributes / hipLaunchKernel).
#pragma once
#include "kernels.h"

namespace eesen {

constexpr int kRecWaves = 8;   // wavefronts per workgroup of every recurrence kernel
// the kernels' workgroup -> role map (struct Role, lstm_persistent.hip), as the launch argument it is: four words
struct RecRole { int nblk, ndir, nz, xcd; };

// the kernel templates; a row's arguments are its template's, in order (bool as 0 / 1)
enum RecFamily { kFwdF32, kFwdBf, kFwdBfGuard, kFwdMux, kBwdGeneric, kBwdQ4, kBwdKsplit, kBwdKsplitH, kBwdKsplitMux };
struct RecKernel {
  int family;
  int kind;          // kRec*: what RecPlan::kind reports, and the launcher's argument list
  int arg[5];
  const void* fn;    // host stub
  const char* name;  // e.g. "lstm_fwd_persistent_kernel<4,1,4,false,true>"
};
// the row of an instantiation; null: there is none
const RecKernel* rec_kernel(int family, int a0, int a1 = 0, int a2 = 0, int a3 = 0, int a4 = 0);
// host stubs of the two utility kernels the planner launches
const void* handoff_pingpong_fn();   // (unsigned* flags, unsigned long long* out, int rounds), 2 workgroups of 64
const void* wait_for_word_fn();      // (const unsigned* word, unsigned target, unsigned* err, unsigned long long limit_ticks), one wave

}  // namespace eesen
