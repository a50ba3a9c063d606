# tests/host_sim/dedup_plan.mk: the class plan of the equal-range finder (nlzm_amd/csrc/nlzm_dedup_plan.h) in a program of its own, under
# AddressSanitizer and UBSan.  TEST HARNESS ONLY (tests/test_dedup_plan.py).
DEPS = dedup_plan_sim.cpp ../../nlzm_amd/csrc/nlzm_dedup_plan.h ../../nlzm_amd/csrc/nlzm_read_plan.h ../../nlzm_amd/csrc/nlzm_units.h ../../include/nlzm_hip.h
all: dedup_plan_sim_san
dedup_plan_sim_san: $(DEPS)
	g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ dedup_plan_sim.cpp
clean:
	rm -f dedup_plan_sim_san
