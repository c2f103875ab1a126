// K1 for 4-byte pixels (RGBA8, BGRA8) through the context's per-channel lookup tables (jpge_set_channel_lut): fdct.hip built with that load shape and the table map in the staging (see "channel tables" there).
#define JPGE_K1_SHAPE 2
#define JPGE_K1_LUT 1
#define JPGE_K1_ENTRY launch_fdct_x4_lut
#include "fdct.hip"
