// K1 for 4-byte pixels (RGBA8, BGRA8), oriented, mirrored (JPGE_ORIENT_FLIP_H, _ROT180): fdct.hip built with that load shape and orientation class (see "oriented loads" there).
#define JPGE_K1_SHAPE 2
#define JPGE_K1_ORIENT 2
#define JPGE_K1_ENTRY launch_fdct_x4_o2
#include "fdct.hip"
