// K1 for v210 (10-bit 4:2:2, three samples to a 32-bit word, six pixels in 16 bytes): fdct.hip built with that load shape (see "input layouts" there).
#define JPGE_K1_SHAPE 16
#define JPGE_K1_ENTRY launch_fdct_v210
#include "fdct.hip"
