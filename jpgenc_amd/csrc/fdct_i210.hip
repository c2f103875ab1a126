// K1 for I210 (10-bit 4:2:2 in 16-bit words: Y, Cb, Cr planes, a chroma row per pixel row): fdct.hip built with that load shape (see "input layouts" there).
#define JPGE_K1_SHAPE 15
#define JPGE_K1_ENTRY launch_fdct_i210
#include "fdct.hip"
