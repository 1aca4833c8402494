// The mel plan (pe_mel_plan_create, mel.hip) as the forward (mel.hip) and the backward (mel_grad.hip) see it.
#pragma once
#include "common.h"

// Opens with six ints: the host checks of the backward entry points read `hop` alone before anything else of the
// plan, so a test without a device reaches them with a host-only header (tests/test_mel_grad_cpu.py).
struct pe_mel_plan {
  int sample_rate, n_fft, hop, n_mels, n_freq, n_pairs;
  void* d_base;
  float* d_win;                // [1024] periodic Hann
  float2* d_tw512;             // [512]  exp(-2 pi i k / 512)
  float2* d_tw1024;            // [257]  exp(-2 pi i k / 1024)
  int* d_fb_idx;               // [n_pairs] first bin of each 8-tap chunk | [n_mels] first chunk | [n_mels] #chunks
  float* d_fb_w;               // [n_pairs][8] chunk weights, zero padded
  // the filterbank transposed, for the backward: bin k has weight d_tfb_w[k].x in filter d_tfb_m[k].x and .y in .y
  // (ascending filters; an unused slot is filter 0 with weight 0).  Null when some bin has more than two filters.
  int2* d_tfb_m;               // [513]
  float2* d_tfb_w;             // [513]
};
