// fs2_modspec.h - the sizes of the modulation spectrum, one set for the over-smoothing scores (fs2_modspec.hip) and the postfilter
// (fs2_msfilter.hip), which transforms the same trajectories on the same frequency grid.
#pragma once
#include "fs2_comp.h"

#define MS_NFFT 4096
#define MS_HALF (MS_NFFT / 2)
#define MS_MAX_FRAMES 2048          // = fs2_dtw_max_frames(): N is twice the frame bound
#define MS_MAX_K 128
#define MS_NT 256
