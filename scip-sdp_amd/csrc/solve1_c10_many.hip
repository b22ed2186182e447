/* solve1_c10_many.hip - the one-launch node solve (csrc/solve1_body.h) for many problems at once (hipsdp_solve_many): instance for
 * problems whose blocks all have at most 10 rows, m <= 64 (256 threads, as solve1_c10.hip); one workgroup per problem, the
 * arguments in device memory */
#define S1_NT 256
#define S1_NW 4
#define S1_NCLS 10
#define S1_MBIG 0
#define S1_MANY
#define S1_KERNEL k_solve1_c10_many
#define S1_LAUNCH_MANY hs_solve1_launch_c10_many
#include "solve1_body.h"
