// K1 for 8-bit Bayer mosaics through the context's per-channel lookup tables (jpge_set_channel_lut; the tables act on the demosaiced pixel): fdct.hip built with that load shape and the table map in the staging (see "channel tables" there).
#define JPGE_K1_SHAPE 17
#define JPGE_K1_LUT 1
#define JPGE_K1_ENTRY launch_fdct_bayer8_lut
#include "fdct.hip"
