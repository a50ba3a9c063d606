// stream_plan_sim.cpp -- the single stream's launch plan (nlzm_amd/csrc/nlzm_stream_plan.h) on its own: no device, no library.
// TEST HARNESS ONLY (tests/test_stream_plan.py; built by the Makefile with -fsanitize=address,undefined).
//
//   stream_plan_sim plan <free_bytes> <table_bytes> <per_chunk> <batch> <nchunks>     one plan, printed: "plan <batch> <depth>"
#include "../../nlzm_amd/csrc/nlzm_stream_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int main(int argc, char **argv)
{
    if (argc == 7 && !strcmp(argv[1], "plan")) {
        const nlzm::stream_plan::Plan P = nlzm::stream_plan::make_plan(atof(argv[2]), atof(argv[3]), atof(argv[4]), (uint32_t)strtoul(argv[5], nullptr, 10),
                                                                       (uint32_t)strtoul(argv[6], nullptr, 10));
        printf("plan %u %u\n", P.batch, P.depth);
        printf("stream_plan_sim: OK\n");
        return 0;
    }
    fprintf(stderr, "usage: stream_plan_sim plan <free_bytes> <table_bytes> <per_chunk> <batch> <nchunks>\n");
    return 2;
}
