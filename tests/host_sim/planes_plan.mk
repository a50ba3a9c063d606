# tests/host_sim/planes_plan.mk: the host plan of the byte-plane filter (nlzm_amd/csrc/nlzm_planes_plan.h) in a program of its own, under
# AddressSanitizer and UBSan.  TEST HARNESS ONLY (tests/test_planes_plan.py).
DEPS = planes_plan_sim.cpp ../../nlzm_amd/csrc/nlzm_planes_plan.h ../../nlzm_amd/csrc/nlzm_read_plan.h ../../nlzm_amd/csrc/nlzm_units.h ../../include/nlzm_hip.h
all: planes_plan_sim_san
planes_plan_sim_san: $(DEPS)
	g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ planes_plan_sim.cpp
clean:
	rm -f planes_plan_sim_san
