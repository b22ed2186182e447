/* solve1_c16_many.hip - the one-launch node solve (csrc/solve1_body.h) for many problems at once (hipsdp_solve_many): instance for
 * problems whose blocks all have at most 16 rows, m <= 64; one workgroup per problem, the arguments in device memory */
#define S1_NCLS 16
#define S1_MBIG 0
#define S1_MANY
#define S1_KERNEL k_solve1_c16_many
#define S1_LAUNCH_MANY hs_solve1_launch_c16_many
#include "solve1_body.h"
