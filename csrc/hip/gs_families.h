// One host launcher per E-step kernel family, private to csrc/hip/*.hip (the public interface is kernels.h
// launch_gs_estep, lda_gs64.hip, which validates the arguments and picks the family by variant).  Each launcher
// owns its switch over the compiled KS and its choice of template instantiation; a.n_items > 0.
#pragma once
#include "kernels.h"

namespace oni {

// gs_short.hip
void launch_gs_tiny(const GSArgs& a, int KS, hipStream_t s);
void launch_gs_small(const GSArgs& a, int KS, hipStream_t s);   // KS > 32: gs_smallw
void launch_gs_chain(const GSArgs& a, int KS, hipStream_t s);
// gs_team.hip: NW = 1, 4 or 8 waves per document (KS <= 32 at U <= kGsUMax: NW = 1 only, else gs_wteam.hip)
void launch_gs_team(const GSArgs& a, int KS, int NW, hipStream_t s);
// gs_wteam.hip (KS <= 32, U <= kGsUMax): one wave per document / 7 word waves + a topic wave
void launch_gs_wteam(const GSArgs& a, int KS, hipStream_t s);
void launch_gs_wsteam(const GSArgs& a, int KS, hipStream_t s);

}  // namespace oni
