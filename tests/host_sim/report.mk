# tests/host_sim/report.mk: the compress pipeline's reports (nlzm_amd/csrc/nlzm_report.h) on synthetic structs, under UBSan and
# AddressSanitizer (no fibers here, so both).  TEST HARNESS ONLY.
SRC  = report_sim.cpp
DEPS = $(SRC) ../../nlzm_amd/csrc/nlzm_report.h ../../nlzm_amd/csrc/nlzm_v2.h ../../nlzm_amd/csrc/nlzm_core.h ../../nlzm_amd/csrc/xw.h
CXXFLAGS = -O1 -g -std=c++17 -Wall -Wno-unknown-pragmas -Wno-unused-function -Wno-unused-variable -Wno-unused-but-set-variable
all: report_sim_san
report_sim_san: $(DEPS)
	g++ $(CXXFLAGS) -fsanitize=undefined,address -fno-sanitize-recover=undefined -o $@ $(SRC)
clean:
	rm -f report_sim_san
