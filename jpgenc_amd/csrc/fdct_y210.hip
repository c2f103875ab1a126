// K1 for Y210 (10-bit 4:2:2 in 16-bit words: packed groups Y0 Cb Y1 Cr): fdct.hip built with that load shape (see "input layouts" there).
#define JPGE_K1_SHAPE 13
#define JPGE_K1_ENTRY launch_fdct_y210
#include "fdct.hip"
