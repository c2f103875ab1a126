// K1 for RGB8, oriented, transposed (JPGE_ORIENT_TRANSPOSE, _ROT90): fdct.hip built with that load shape and orientation class (see "oriented loads" there).
#define JPGE_K1_SHAPE 0
#define JPGE_K1_ORIENT 3
#define JPGE_K1_ENTRY launch_fdct_rgb8_o3
#include "fdct.hip"
