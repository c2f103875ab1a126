// K1 for RGBA8 / BGRA8, box downscale by 4 (jpge_set_downscale): fdct.hip built with that load shape and factor (see "downscaling loads" there).
#define JPGE_K1_SHAPE 2
#define JPGE_K1_DS 4
#define JPGE_K1_ENTRY launch_fdct_x4_d4
#include "fdct.hip"
