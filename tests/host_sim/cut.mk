# tests/host_sim/cut.mk: the cut-point roles (nlzm_amd/csrc/nlzm_cut.h) run on the CPU, every lane a fiber (xw_sim.cpp), under UBSan as
# crc_sim_san is (AddressSanitizer does not follow the fibers' hand-switched stacks: the harness puts PROT_NONE pages round the input
# and guard words behind every output instead).  TEST HARNESS ONLY.
SRC  = cut_sim.cpp xw_sim.cpp
DEPS = $(SRC) ../../nlzm_amd/csrc/nlzm_cut.h ../../nlzm_amd/csrc/xw.h
CXXFLAGS = -O2 -g -std=c++17 -Wall -Wno-unknown-pragmas -Wno-unused-function
all: cut_sim_san
cut_sim_san: $(DEPS)
	g++ $(CXXFLAGS) -fsanitize=undefined -fno-sanitize-recover=undefined -o $@ $(SRC)
clean:
	rm -f cut_sim_san
