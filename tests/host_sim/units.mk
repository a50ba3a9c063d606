# tests/host_sim/units.mk: the unit table of the range kernels (nlzm_amd/csrc/nlzm_units.h: count, prefix, owner_of, blocks_for) in a program of its
# own, under AddressSanitizer and UBSan.  TEST HARNESS ONLY (tests/test_units_sim.py).
DEPS = units_sim.cpp ../../nlzm_amd/csrc/nlzm_units.h
all: units_sim_san
units_sim_san: $(DEPS)
	g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ units_sim.cpp
clean:
	rm -f units_sim_san
