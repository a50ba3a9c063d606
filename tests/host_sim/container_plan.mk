# tests/host_sim/container_plan.mk: the plan of a container compressed in sets (nlzm_amd/csrc/nlzm_container_plan.h) in a program of its
# own, under AddressSanitizer and UBSan.  TEST HARNESS ONLY (tests/test_container_plan.py).
DEPS = container_plan_sim.cpp ../../nlzm_amd/csrc/nlzm_container_plan.h ../../nlzm_amd/csrc/nlzm_read_plan.h ../../nlzm_amd/csrc/nlzm_units.h ../../include/nlzm_hip.h
all: container_plan_sim_san
container_plan_sim_san: $(DEPS)
	g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ container_plan_sim.cpp
clean:
	rm -f container_plan_sim_san
