// sx_tables.h -- the plain structs and limits the host table builders (sx_tablehost.h) and the kernels that read their tables
// (sx_prcpindices.h, sx_resident.h) share.  No HIP: a plain C++ compiler can include this file.
#pragma once

#define SX_RES_MAXCELLS 1024                // sx_k_res_fwd: one cell per thread, one workgroup per sample

#define SX_PI_NQ 11                         // quantiles 0, 0.1 .. 1

struct SxPiGauge {
    int lb;                                 // first entry of the gauge in the list (a multiple of 64)
    int db;                                 // first entry of its catchment in the distance arrays (a multiple of 64)
    int sec[SX_PI_NQ + 1];                  // section s is blocks [sec[s], sec[s + 1]) of the gauge
    float wf[SX_PI_NQ];
    float cnt[SX_PI_NQ];                    // cnt[k], k = 1 .. 10: real(count(mask_k)); cnt[0] unused
    int krr;                                // plan cell of (gauge_row, gauge_row)
};
