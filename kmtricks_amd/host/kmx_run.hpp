// kmx_run.hpp -- what the commands of `kmx` that lay out a run directory share: the fof grammar, the directory tree, the way out on an error.
#pragma once
#include <filesystem>
#include <fstream>
#include <iostream>
#include <map>
#include <regex>
#include <sstream>
#include <string>
#include <vector>
#include <unistd.h>

struct Sample { std::string id; std::vector<std::string> files; uint32_t hard_min; };


// (a worker thread cannot unwind the others: print and leave without running destructors under them)
[[noreturn]] inline void die(const std::string& msg) { std::cerr << "[error] " << msg << std::endl; std::cerr.flush(); _exit(EXIT_FAILURE); }

inline std::vector<Sample> parse_fof(const std::string& path, uint32_t default_hard_min)
{ // grammar `ID : path[ ; path...][ ! hardmin]` (io/fof.hpp:39-43, 126-134)
  std::ifstream in(path); if (!in) die("Unable to read at " + path);
  static const std::regex pat(R"((^[A-Za-z0-9_-]+)[\s]*:[\s]*([.A-Za-z0-9\/_\-; ]+)([\s]*![\s]*)?([0-9]+$)?)");
  std::vector<Sample> out; std::map<std::string, int> seen; std::string line;
  namespace fs = std::filesystem;
  const fs::path base = fs::absolute(fs::path(path)).parent_path();
  while (std::getline(in, line)) {
    while (!line.empty() && (line.back() == '\r' || line.back() == ' ')) line.pop_back();
    if (line.empty()) continue;
    std::smatch m;
    if (!std::regex_match(line, m, pat)) die("fof: invalid line: " + line);
    Sample s; s.id = m[1]; s.hard_min = m[4].matched ? (uint32_t)std::stoul(m[4]) : default_hard_min;
    if (seen[s.id]++) die("fof: duplicate id " + s.id);
    std::stringstream ss(m[2]); std::string f;
    while (std::getline(ss, f, ';')) {
      f.erase(0, f.find_first_not_of(" \t")); f.erase(f.find_last_not_of(" \t") + 1);
      if (f.empty()) continue;
      fs::path p(f); if (p.is_relative() && !fs::exists(p)) p = base / p;   // fixtures use paths relative to the fof
      s.files.push_back(p.string());
    }
    if (s.files.empty()) die("fof: no file for " + s.id);
    out.push_back(s);
  }
  if (out.empty()) die("fof: empty");
  return out;
}


// the run directory (kmdir.hpp:195-241)
inline void make_run_layout(const std::string& root)
{
  for (const char* d : {"", "/superkmers", "/counts", "/matrices", "/filters", "/histograms", "/merge_infos", "/howde_index",
                        "/partition_infos", "/fpr", "/plugin_output", "/repartition_gatb", "/config_gatb"})
    std::filesystem::create_directories(root + d);
}
