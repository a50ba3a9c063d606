# tests/host_sim/far.mk: the CRC32, equal-range and byte-plane roles at offsets on either side of 2^32 of one sparse mapping, run on the CPU, every
# lane a fiber (xw_sim.cpp), under UBSan as dedup_sim_san is (AddressSanitizer does not follow the fibers' hand-switched stacks).  TEST HARNESS ONLY.
CSRC = ../../nlzm_amd/csrc
SRC  = far_sim.cpp xw_sim.cpp
DEPS = $(SRC) $(CSRC)/nlzm_crc.h $(CSRC)/nlzm_dedup.h $(CSRC)/nlzm_planes.h $(CSRC)/nlzm_range.h $(CSRC)/nlzm_dedup_plan.h $(CSRC)/nlzm_planes_plan.h $(CSRC)/nlzm_read_plan.h $(CSRC)/nlzm_units.h $(CSRC)/xw.h
CXXFLAGS = -O2 -g -std=c++17 -Wall -Wno-unknown-pragmas -Wno-unused-function
all: far_sim_san
far_sim_san: $(DEPS)
	g++ $(CXXFLAGS) -fsanitize=undefined -fno-sanitize-recover=undefined -o $@ $(SRC)
clean:
	rm -f far_sim_san
