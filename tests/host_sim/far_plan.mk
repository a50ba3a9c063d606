# tests/host_sim/far_plan.mk: the range entry points' host tables (crc::SegTable, planes::Table and Layout, make_ranges_plan, units::prefix) for
# ranges longer than 2^32 in a program of its own, under AddressSanitizer and UBSan.  TEST HARNESS ONLY (tests/test_far_plan.py).
CSRC = ../../nlzm_amd/csrc
DEPS = far_plan_sim.cpp $(CSRC)/nlzm_container_plan.h $(CSRC)/nlzm_dedup_plan.h $(CSRC)/nlzm_planes_plan.h $(CSRC)/nlzm_read_plan.h $(CSRC)/nlzm_units.h ../../include/nlzm_hip.h
all: far_plan_sim_san
far_plan_sim_san: $(DEPS)
	g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ far_plan_sim.cpp
clean:
	rm -f far_plan_sim_san
