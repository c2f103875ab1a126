// K1 for planar R, G, B (RGB8_PLANAR): fdct.hip built with that load shape (see "input layouts" there).
#define JPGE_K1_SHAPE 3
#define JPGE_K1_ENTRY launch_fdct_planar
#include "fdct.hip"
