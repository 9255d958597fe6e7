// avz_chunked_k.hpp — kernels of the chunk-parallel form of the mask-driven MVDR chain (gfx950).
//
// An utterance's frames are cut into 32-frame chunks; each (chunk, utterance) pair is
// one 256-thread (4-wave) workgroup, two per CU, so a batch of B utterances of T
// frames launches B * ceil(T / 32) independent blocks instead of B long ones.
//
//   analysis   frames -> window -> FFT (mic pair / reference pair packed) -> LDS;
//              thread-per-bin masks (IBM / IPD / external) and masked 2x2 covariance
//              partials over the chunk (fp32) -> part[b][c][5][F]; IBM bits -> mwords.
//   solve      one thread per (utterance, bin): partials summed in fp64, closed-form
//              2x2 MVDR with the plan's steering table -> coef[b][k] (alpha, beta).
//   synthesis  frames -> FFT again -> apply w^H y +
//              post-filter -> two frames packed per inverse FFT -> windowed OLA of the
//              chunk's 31 interior segments -> out; the chunk's first / last
//              half-frame contributions -> heads/tails;
//              block max |out| -> atomicMax(peak_u[b]).
//   finalize   chunk-boundary segments (tails[c-1] + heads[c]), utterance peak,
//              optional in-place peak normalisation of the chunk's segments.
//
// Reference semantics as avz_kernels.hip: rt_av_zoom/core/oracle_debug.py:27-97,
// rt_av_zoom/core/masked_mvdr.py:50-132,
// rt_av_zoom/core/full_audio_generating_pipeline/inference.py:88-118.
// The kernels are in one header per stage, included here in order.
#pragma once
#include "avz_chain_common.hpp"     // geometry, window + FFT helpers, IBM decision, KArgs
#include "avz_chain_exact.hpp"      // the analysis kernel's exact-IBM path
#include "avz_chain_analysis.hpp"   // avz_analysis_kernel
#include "avz_chain_solve.hpp"      // avz_solve*_kernel, avz_srp_kernel
#include "avz_chain_synthesis.hpp"  // avz_synthesis_kernel (chunk grid)
#include "avz_chain_utt.hpp"        // avz_synthesis_utt_kernel, _utt512_kernel (whole utterances)
#include "avz_chain_finalize.hpp"   // avz_finalize_kernel, avz_finalize_pieces_kernel
