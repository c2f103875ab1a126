// K1 for BGR8, box downscale by 2 (jpge_set_downscale): fdct.hip built with that load shape and factor (see "downscaling loads" there).
#define JPGE_K1_SHAPE 1
#define JPGE_K1_DS 2
#define JPGE_K1_ENTRY launch_fdct_bgr8_d2
#include "fdct.hip"
