// K1 for NV12, box downscale by 4 (jpge_set_downscale): fdct.hip built with that load shape and factor (see "downscaling loads" there).
#define JPGE_K1_SHAPE 4
#define JPGE_K1_DS 4
#define JPGE_K1_ENTRY launch_fdct_nv12_d4
#include "fdct.hip"
