// qc_ref_driver.cpp -- TEST INFRASTRUCTURE ONLY (build container; tests/golden/make_qc_goldens.py).
//
// Own code (not copied from the reference).  It links against the reference's own Statistics and
// MeasureCoverage modules, compiled in place from the reference's sources, and wires the chains the reference's
// commands build (commands/command_stats.cpp, command_coverage.cpp):
//   stats in.bam                              FileReader -> Statistics, both summaries on (-I -L)
//   coverage in.bam out.tsv BINSIZE zero|nz   FileReader -> MeasureCoverage, with or without uncovered bins
// The module's own stdout / stderr are what the recipe records.  Never part of the product and never run by
// a test.
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>

#include "algorithms/algorithm_module.h"
#include "algorithms/file_reader.h"
#include "algorithms/measure_coverage.h"
#include "algorithms/statistics.h"

int main(int argc, char **argv) {
    if (argc < 3) {
        std::cerr << "usage: qc_ref_driver stats in.bam | coverage in.bam out.tsv binsize zero|nz" << std::endl;
        return 2;
    }
    const std::string mode = argv[1];
    OGEParallelismSettings::setNumberThreads(4);
    AlgorithmModule::setNothreads(false);
    AlgorithmModule::setVerbose(false);
    OGEParallelismSettings::enableMultithreading();
    FileReader reader;
    reader.addFile(argv[2]);
    if (mode == "stats") {
        Statistics s;
        s.showInsertSizeSummary(true);
        s.showReadLengthSummary(true);
        reader.addSink(&s);
        reader.runChain();
    } else if (mode == "coverage" && argc == 6) {
        reader.setLoadStringData(false);
        MeasureCoverage c;
        c.setOutputFile(argv[3]);
        c.setVerifyCorrectMapping(false);
        c.setPrintZeroCoverageBases(strcmp(argv[5], "zero") == 0);
        c.setBinSize(atoi(argv[4]));
        c.setStrict(false);
        reader.addSink(&c);
        reader.runChain();
    } else {
        return 2;
    }
    std::cout.flush();
    OGERead::clearCachedAllocations();
    ThreadPool::closeSharedPool();
    return 0;
}
