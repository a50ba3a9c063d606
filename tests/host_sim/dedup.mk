# tests/host_sim/dedup.mk: the equal-range finder's roles (nlzm_amd/csrc/nlzm_dedup.h) run on the CPU, every lane a fiber (xw_sim.cpp), under UBSan
# as cut_sim_san is (AddressSanitizer does not follow the fibers' hand-switched stacks: the harness puts PROT_NONE pages round the bytes that are
# read and guard words behind every output instead).  TEST HARNESS ONLY.
SRC  = dedup_sim.cpp xw_sim.cpp
DEPS = $(SRC) ../../nlzm_amd/csrc/nlzm_dedup.h ../../nlzm_amd/csrc/nlzm_units.h ../../nlzm_amd/csrc/xw.h
CXXFLAGS = -O2 -g -std=c++17 -Wall -Wno-unknown-pragmas -Wno-unused-function
all: dedup_sim_san
dedup_sim_san: $(DEPS)
	g++ $(CXXFLAGS) -fsanitize=undefined -fno-sanitize-recover=undefined -o $@ $(SRC)
clean:
	rm -f dedup_sim_san
