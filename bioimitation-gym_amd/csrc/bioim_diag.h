// bioim_diag.h — the diagnostic builds' device globals and stamp macros
// (-DBIOIM_STAMPS, -DBIOIM_WAVETIME: whole-translation-unit builds, never
// shipped).  Without those defines this header declares nothing and STAMP /
// STAMP_DECL expand to nothing.
#pragma once

#include <hip/hip_runtime.h>

#include "bioim_config.h"

#ifdef BIOIM_STAMPS
__device__ unsigned long long g_stamps[28];
#endif
/* Diagnostic build only (-DBIOIM_WAVETIME, single translation unit,
 * tools/wavetime.py): shader cycles of every wave of the last step launch */
#ifdef BIOIM_WAVETIME
#define BIOIM_WAVETIME_N 65536
__device__ unsigned long long g_wavetime[BIOIM_WAVETIME_N];
/* per thread of the last launch: fiber-velocity Newton iterations (sum over
 * the launch's solves), the most of one solve, bisection fallbacks */
__device__ unsigned g_fvit[BIOIM_WAVETIME_N * 4], g_fvmax[BIOIM_WAVETIME_N * 4], g_fvbis[BIOIM_WAVETIME_N * 4];
DEV unsigned diag_tid() { return blockIdx.x * blockDim.x + threadIdx.x; }
#endif

/* Diagnostic build only (-DBIOIM_STAMPS, tools/stamps.py): per-phase shader
 * cycles of the first env of workgroup 0, accumulated over one launch. */
#ifdef BIOIM_STAMPS
#define STAMP(i)                                                                      \
    do {                                                                              \
        __builtin_amdgcn_sched_barrier(0);                                            \
        unsigned long long t_ = __builtin_amdgcn_s_memtime();                         \
        __builtin_amdgcn_s_waitcnt(0xC07F);                                           \
        if (blockIdx.x == 0 && threadIdx.x == 0) g_stamps[i] += t_ - stamp_prev;      \
        stamp_prev = t_;                                                              \
        __builtin_amdgcn_sched_barrier(0);                                            \
    } while (0)
#define STAMP_DECL unsigned long long stamp_prev = __builtin_amdgcn_s_memtime();
#else
#define STAMP(i) do {} while (0)
#define STAMP_DECL
#endif
