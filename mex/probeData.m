function probeData(varargin)
% Drop-in for include/probeData.m of either receiver: figure 100 with the time-domain
% excerpt, the Welch PSD and the histogram of the start of an IF record.  The numbers
% come from the GPU (bds_mex('probe_data', ...) -> bds_probe_data_file of
% libbds_mi355x.so); this file only draws them.
%
%   probeData(settings)              the record is settings.fileName
%   probeData(fileName, settings)
%
% Beyond the reference: packed records (settings.fileType 3) are read too.
% settings.skipNumberOfBytes counts samples, as in tracking (the same number for an
% int8 real record).
switch nargin
    case 1
        settings = varargin{1};
        fileNameStr = settings.fileName;
    case 2
        fileNameStr = varargin{1};
        settings = varargin{2};
        if ~ischar(fileNameStr), error('File name must be a string'); end
    otherwise
        error('Incorect number of arguments');
end
signal = 2 - isfield(settings, 'acqCohT');   % only B1C/initSettings.m defines acqCohT: 1 = B1C, 2 = B2a
p = bds_mex('probe_data', fileNameStr, settings, signal);

fs = settings.samplingFreq;
iq = settings.fileType ~= 1;
rows = 2 + iq;                                % 2 x 2 panels for a real record, 3 x 2 for I/Q
t_ms = 1e3 * (0:numel(p.excerpt_re) - 1) / fs;
nb = numel(p.psd);
span = max(abs(p.stats([1 2 5 6]))) + 1;      % max(abs(data)) + 1 of the histogram axes

figure(100); clf(100);

% frequency domain: the top row
subplot(rows, 2, 1:2);
if iq
    % two-sided density, 0 .. fs in natural order -> -fs/2 .. fs/2, in dB
    f = (0:nb - 1).' * (fs / nb);
    half = nb / 2;
    plot([-flipud(f(1:half)); f(1:half)] / 1e6, 10 * log10([p.psd(half + 1:end); p.psd(1:half)]));
    ylabel('Magnitude');
else
    % one-sided density per Hz; the reference hands pwelch fs / 1e6, whose own plot is then in dB per MHz
    plot((0:nb - 1).' * (fs / 1e6) / (2 * (nb - 1)), 10 * log10(p.psd * 1e6));
    ylabel('Power/frequency (dB/MHz)');
end
decorate('Frequency domain plot', 'Frequency (MHz)', '');

% time domain and histograms
if iq
    panel_time(subplot(rows, 2, 4), t_ms, p.excerpt_re, 'Time domain plot (I)');
    panel_time(subplot(rows, 2, 3), t_ms, p.excerpt_im, 'Time domain plot (Q)');
    panel_hist(subplot(rows, 2, 6), p.hist_i, span, 'Histogram (I)');
    panel_hist(subplot(rows, 2, 5), p.hist_q, span, 'Histogram (Q)');
else
    panel_time(subplot(rows, 2, 3), t_ms, p.excerpt_re, 'Time domain plot');
    panel_hist(subplot(rows, 2, 4), p.hist_i, span, 'Histogram');
end
end

function decorate(name, xl, yl)
axis tight; grid on; title(name); xlabel(xl);
if ~isempty(yl), ylabel(yl); end
end

function panel_time(ax, t_ms, v, name)
axes(ax); %#ok<LAXES>
plot(t_ms, v);
decorate(name, 'Time (ms)', 'Amplitude');
end

function panel_hist(ax, counts, span, name)
axes(ax); %#ok<LAXES>
bar(-128:128, counts, 1);
decorate(name, 'Bin', 'Number in bin');
lim = axis;
axis([-span span lim(3:4)]);
end
