// afv_essgraph.h — what afv_essgraph.hip (host side) and k_essgraph.hip (kernels) share beyond afv_essgraph_math.h
#pragma once

#include "afv_essgraph_math.h"

struct DevEssCorrect {       // k_ess_correct_points: a kernel argument
    float *pos[3];           // the store's position planes
    const uint8_t *flags;
    const int *ids, *pair;   // [n]; pair: a position in S_from / S_to, -1: none
    const double *S_from, *S_to;  // [m][13]
    double *xyz_out;         // [n][3] or null
    uint8_t *status;         // [n]
    int n, write_points;
};

extern "C" void afv_launch_ess_round(const EgView *V, int max_it, hipStream_t stream);
extern "C" void afv_launch_ess_iteration(const EgView *V, double lambda_init, hipStream_t stream);  // perturb, linearise, terms, build, begin
extern "C" void afv_launch_ess_trial(const EgView *V, hipStream_t stream);                          // load, factor, step, trial, judge
extern "C" void afv_launch_ess_recover(const EgView *V, double *S_out, double *Tiw, double *Swc, hipStream_t stream);
extern "C" void afv_launch_ess_correct_points(const DevEssCorrect *J, hipStream_t stream);
