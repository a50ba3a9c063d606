# tests/host_sim/ranges_plan.mk: the plan of a call on ranges of the caller's choosing (nlzm_amd/csrc/nlzm_container_plan.h, make_ranges_plan)
# in a program of its own, under AddressSanitizer and UBSan.  TEST HARNESS ONLY (tests/test_ranges_plan.py).
DEPS = ranges_plan_sim.cpp ../../nlzm_amd/csrc/nlzm_container_plan.h ../../nlzm_amd/csrc/nlzm_read_plan.h ../../nlzm_amd/csrc/nlzm_units.h ../../include/nlzm_hip.h
all: ranges_plan_sim_san
ranges_plan_sim_san: $(DEPS)
	g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ ranges_plan_sim.cpp
clean:
	rm -f ranges_plan_sim_san
