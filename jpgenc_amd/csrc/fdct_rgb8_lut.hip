// K1 for RGB8 through the context's per-channel lookup tables (jpge_set_channel_lut): fdct.hip built with that load shape and the table map in the staging (see "channel tables" there).
#define JPGE_K1_SHAPE 0
#define JPGE_K1_LUT 1
#define JPGE_K1_ENTRY launch_fdct_rgb8_lut
#include "fdct.hip"
